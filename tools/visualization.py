"""A coloured point cloud of one room of a test run's --out directory (softgroup_amd.util.visualize), as an
ASCII PLY file or in an open3d window.

    python tools/visualization.py --prediction_path results --room_name scene0011_00 --task instance_pred --out a.ply
    python tools/visualization.py --prediction_path results --all-rooms --out-dir clouds [--task instance_pred]

Tasks: input, semantic_gt, semantic_pred, offset_semantic_pred, instance_gt, instance_pred.  With --all-rooms
every room that has a coords file is written to <out-dir>/<room>_<task>.ply.
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd.util import visualize as V  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--prediction_path', default='./results', help="the test run's --out directory")
    ap.add_argument('--room_name', default='scene0011_00', help='scan to draw (file stem under <prediction_path>/coords)')
    ap.add_argument('--task', default='instance_pred', choices=V.TASKS, help='what the colours show')
    ap.add_argument('--out', help='write the cloud to this .ply file; without it a viewer window opens')
    ap.add_argument('--backend', default='auto', choices=('auto', 'device', 'numpy'))
    ap.add_argument('--all-rooms', action='store_true', help='every room of the prediction path, into --out-dir')
    ap.add_argument('--out-dir', help='directory of the PLY files of --all-rooms')
    return ap.parse_args(argv)


def rooms_of(prediction_path):
    coords = os.path.join(prediction_path, 'coords')
    return sorted(f[:-4] for f in os.listdir(coords) if f.endswith('.npy')) if os.path.isdir(coords) else []


def show(xyz, rgb):
    """hands the arrays to open3d's stock viewer: float64 positions, colours in 0..1"""
    import open3d as o3d
    cloud = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(xyz[:, :3].astype('float64')))
    cloud.colors = o3d.utility.Vector3dVector(rgb.astype('float64') / 255)
    o3d.visualization.draw_geometries([cloud])


def main(argv=None):
    opt = parse_args(argv)
    if opt.all_rooms:
        if not opt.out_dir:
            sys.exit('--all-rooms writes one file per room: give --out-dir')
        rooms = rooms_of(opt.prediction_path)
        if not rooms:
            sys.exit(f'no rooms under {opt.prediction_path}/coords')
        for info in V.save_visualizations(opt.prediction_path, rooms, [opt.task], opt.out_dir, backend=opt.backend):
            print('%s: %d vertices' % (info['path'], info['vertices']))
        return 0
    if opt.out:
        if not opt.out.endswith('.ply'):
            sys.exit(f'--out {opt.out}: the cloud is written as ASCII PLY, so name it something.ply')
        out_dir = os.path.dirname(os.path.abspath(opt.out))
        os.makedirs(out_dir, exist_ok=True)
        with tempfile.TemporaryDirectory(dir=out_dir) as scratch:      # (no generated name can meet a file of the user's)
            info, = V.save_visualizations(opt.prediction_path, [opt.room_name], [opt.task], scratch, backend=opt.backend)
            os.replace(info['path'], os.path.abspath(opt.out))
        print('%s: %d vertices' % (opt.out, info['vertices']))
        return 0
    try:
        import open3d  # noqa: F401
    except ImportError:
        sys.exit('open3d is not installed, so there is no window to open: give --out FILE.ply')
    xyz, rgb = V.get_coords_color(opt.prediction_path, opt.room_name, opt.task, backend=opt.backend)
    show(xyz, rgb)
    return 0


if __name__ == '__main__':
    sys.exit(main())
