"""Pictures of a test run's --out directory, or of a raw point-cloud file, as PNG images
(softgroup_amd.util.render): no desktop and no viewer needed.

    python tools/render.py --prediction_path results --room_name scene0011_00 --task instance_pred --out a.png
    python tools/render.py --prediction_path results --all-rooms --task semantic_pred instance_pred --out-dir png
    python tools/render.py --cloud room.ply --views iso top --size 1024 768 --edl --out room.png

Tasks: input, semantic_gt, semantic_pred, offset_semantic_pred, instance_gt, instance_pred.  The views (top, front,
side, iso) stand side by side in one file; with --all-rooms every room that has a coords file is written to
<out-dir>/<room>_<task>.png.  A raw file goes through read_cloud (text table, .csv, .ply, KITTI .bin) and is drawn in
its own colours, or in grey when it has none.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd.util import render as R  # noqa: E402
from softgroup_amd.util import visualize as V  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--prediction_path', default='./results', help="the test run's --out directory")
    ap.add_argument('--room_name', help='scan to draw (file stem under <prediction_path>/coords)')
    ap.add_argument('--all-rooms', action='store_true', help='every room of the prediction path, into --out-dir')
    ap.add_argument('--cloud', help='a raw point-cloud file instead of a prediction path')
    ap.add_argument('--task', nargs='+', default=['instance_pred'], choices=V.TASKS, help='what the colours show')
    ap.add_argument('--views', nargs='+', default=['iso'], choices=sorted(R.VIEWS))
    ap.add_argument('--size', nargs=2, type=int, default=[1024, 768], metavar=('W', 'H'), help='of one view')
    radius = ap.add_mutually_exclusive_group()
    radius.add_argument('--point-size', type=int, default=1, help='splat radius in pixels (0 .. 16)')
    radius.add_argument('--world-radius', type=float, help='splat radius in scene units')
    ap.add_argument('--edl', action='store_true', help='eye-dome lighting')
    ap.add_argument('--orthographic', action='store_true')
    ap.add_argument('--backend', default='auto', choices=('auto', 'device', 'numpy'))
    ap.add_argument('--out', help='the PNG file of one room and one task, or of --cloud')
    ap.add_argument('--out-dir', help='directory of the PNG files (several rooms or tasks)')
    return ap.parse_args(argv)


def rooms_of(prediction_path):
    coords = os.path.join(prediction_path, 'coords')
    return sorted(f[:-4] for f in os.listdir(coords) if f.endswith('.npy')) if os.path.isdir(coords) else []


def main(argv=None):
    opt = parse_args(argv)
    kw = dict(views=opt.views, size=tuple(opt.size), point_size=opt.point_size, world_radius=opt.world_radius,
              edl=True if opt.edl else None, backend=opt.backend,
              kind='orthographic' if opt.orthographic else 'perspective')
    if opt.out and not opt.out.endswith('.png'):
        sys.exit(f'--out {opt.out}: the picture is written as PNG, so name it something.png')
    if opt.cloud:
        if not opt.out:
            sys.exit('--cloud draws one picture: give --out FILE.png')
        from softgroup_amd.util import read_cloud
        cloud = read_cloud(opt.cloud, rgb='raw', backend='numpy')
        xyz = np.asarray(cloud['xyz'], np.float32)
        rgb = cloud['rgb'] if 'rgb' in cloud else np.full(xyz.shape, 128, np.uint8)
        image = R.render_cloud(xyz, rgb, **kw)
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        R.write_png(opt.out, R.montage(image, len(opt.views)))
        print('%s: %d points, %d views' % (opt.out, len(xyz), len(opt.views)))
        return 0
    if opt.all_rooms or len(opt.task) > 1 or not opt.out:
        if not opt.out_dir:
            sys.exit('several rooms or tasks make one file each: give --out-dir (or one room, one task and --out)')
        rooms = rooms_of(opt.prediction_path) if opt.all_rooms else [opt.room_name]
        if not rooms or rooms == [None]:
            sys.exit(f'no rooms under {opt.prediction_path}/coords' if opt.all_rooms else 'give --room_name or --all-rooms')
        for info in R.save_renders(opt.prediction_path, rooms, opt.task, opt.out_dir, **kw):
            print('%s: %d points, %d views' % (info['path'], info['points'], info['views']))
        return 0
    if not opt.room_name:
        sys.exit('give --room_name or --all-rooms')
    out_dir = os.path.dirname(os.path.abspath(opt.out))
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory(dir=out_dir) as scratch:          # (no generated name can meet a file of the user's)
        info, = R.save_renders(opt.prediction_path, [opt.room_name], opt.task, scratch, **kw)
        os.replace(info['path'], os.path.abspath(opt.out))
    print('%s: %d points, %d views' % (opt.out, info['points'], info['views']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
