"""Cost of the render stage (softgroup_amd.util.render_cloud / ops.render) on synthetic clouds: synthetic.scene_s2 with
150 k points (ScanNet-like) and 600 k points (STPLS3D-like), 1024 x 768 per view, V = 1 ('iso') and V = 4 ('iso',
'top', 'front', 'side'), perspective cameras fitted to the cloud, the input colours.

Reported per (cloud, V, radius), all in the same run, each the median over --reps runs after a warm-up (min .. max in
brackets); the radius is point_size 0 / 1 / 4 or a world radius of 0.5 % of the box diagonal:
  fill_ms / splat_ms / resolve_ms / shade_ms   the stages of the C entries on arrays already on the device, HIP events
                                               (shade with eye-dome lighting)
  ns_per_pixel      splat_ms over points x views x (2 r + 1)^2, the nominal covered pixels (fixed radii only)
  device_wall_ms    render_cloud(backend='device') on a CUDA cloud, images left on the device, wall time
  numpy_wall_ms     render_cloud(backend='numpy') on the same cloud as numpy arrays, the twins, wall time
  rasterize / shade, device and numpy   ops.render.rasterize and ops.render.shade on their own, numpy arrays in and
                    out under both backends (upload and read-back included), wall time: what decides _AUTO
Per cloud: write_png of the V = 4 sheet on its own, and as the yardstick save_visualizations writing the same scan's
input PLY (numpy backend, what 'auto' selects), wall time.
The two backends must return the same images, index and depth, byte for byte, before anything is timed.

    python tools/render_bench.py [--reps 5] [--out profiles/render_bench.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.ops import render as RO  # noqa: E402
from softgroup_amd.util import render as R  # noqa: E402
from softgroup_amd.util import save_results, save_visualizations  # noqa: E402

CASES = [('scannet', 150000, 1.0), ('stpls3d', 600000, 2.0)]
VIEW_SETS = [('iso',), ('iso', 'top', 'front', 'side')]
SIZE = (1024, 768)
RADII = [('ps0', 0, None), ('ps1', 1, None), ('ps4', 4, None), ('world', 0, 0.005)]


class _Dataset:
    NYU_ID = None


def wall_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def event_ms(fn, reps, before=None):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before is not None:
            before()                                        # (untimed: the state the timed stage starts from)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def cell(ts, digits=3):
    return f'{np.median(ts):.{digits}f} [{min(ts):.{digits}f} .. {max(ts):.{digits}f}]'


def same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ply_yardstick(xyz, rgb, inst, reps):
    """save_visualizations of the scan's input cloud from a save_results tree, wall ms"""
    n = len(xyz)
    result = dict(scan_id='scan', coords_float=xyz, color_feats=rgb, semantic_labels=np.zeros(n, np.int64),
                  semantic_preds=np.zeros(n, np.int64), offset_preds=np.zeros((n, 3), np.float32),
                  offset_labels=np.zeros((n, 3), np.float32), gt_instances=np.maximum(inst, 0).astype(np.int64) + 1001,
                  pred_instances=[])
    with tempfile.TemporaryDirectory() as root:
        save_results(root, [result], ['semantic', 'instance'], _Dataset, backend='numpy')
        fn = lambda: save_visualizations(root, ['scan'], ['input'], os.path.join(root, 'ply'), backend='numpy')  # noqa: E731
        fn()
        return wall_ms(fn, reps, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = [f'# tools/render_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median [min .. max]; '
             f'{SIZE[0]} x {SIZE[1]} per view, perspective, shade with eye-dome lighting',
             f'{"set":8s} {"points":>7s} {"V":>2s} {"radius":>6s} | fill | splat | resolve | shade | ns_per_pixel | '
             f'device_wall | numpy_wall | rasterize device | rasterize numpy | shade device | shade numpy '
             f'(the last four: numpy arrays in and out, wall)']
    rows = []
    for c, (name, n_points, room_scale) in enumerate(CASES):
        xyz, rgb, inst = synthetic.scene_s2(seed=30 + c, n=n_points, room_scale=room_scale)
        xyz = np.ascontiguousarray(xyz, np.float32)
        colors = R._as_uint8((np.asarray(rgb, np.float32) + 1) * 127.5)
        n = xyz.shape[0]
        lo, hi = R.cloud_bounds(xyz)
        diagonal = float(np.sqrt(((hi - lo) ** 2).sum()))
        d_xyz, d_colors = torch.from_numpy(xyz).to(dev), torch.from_numpy(colors).to(dev)
        sheet = None
        for views in VIEW_SETS:
            cams = R.cameras_for(views, lo, hi, SIZE)
            table = torch.from_numpy(RO.camera_table(cams)).to(dev)
            edl = R._edl_params(True, lo, hi)
            for label, point_size, world in RADII:
                world = None if world is None else world * diagonal
                kw = dict(views=views, size=SIZE, point_size=point_size, world_radius=world, edl=True,
                          return_buffers=True)
                want = R.render_cloud(xyz, colors, backend='numpy', **kw)                  # (also the warm-up)
                got = R.render_cloud(d_xyz, d_colors, backend='device', **kw)
                assert all(same(g, w) for g, w in zip(got, want)), (name, views, label)
                if len(views) == 4 and label == 'ps1':
                    sheet = R.montage(want[0], 4)
                device_wall = wall_ms(lambda: R.render_cloud(d_xyz, d_colors, backend='device', **kw), args.reps, True)
                numpy_wall = wall_ms(lambda: R.render_cloud(xyz, colors, backend='numpy', **kw), args.reps, False)
                # the two operations on their own, numpy arrays in and out (what decides ops/render.py: _AUTO)
                ops = {}
                for backend in ('device', 'numpy'):
                    ops['rasterize_' + backend] = wall_ms(lambda: RO.rasterize(
                        xyz, cams, SIZE[0], SIZE[1], point_size, world, backend=backend), args.reps, backend == 'device')
                    ops['shade_' + backend] = wall_ms(lambda: RO.shade(
                        want[1], want[2], colors, (255, 255, 255), edl, backend=backend), args.reps, backend == 'device')
                ps, w = RO._radius(point_size, world)
                bufs = RO.rasterize_device(d_xyz, table, SIZE[0], SIZE[1], ps, w)
                run = lambda s: RO.rasterize_device(d_xyz, table, SIZE[0], SIZE[1], ps, w, s, bufs)  # noqa: E731
                # (every timed splat starts from freshly filled keys: on keys that already hold the minima it would
                # issue no atomic at all)
                stage = [event_ms(lambda: run(1), args.reps), event_ms(lambda: run(2), args.reps, lambda: run(1)),
                         event_ms(lambda: run(4), args.reps)]
                stage.append(event_ms(lambda: RO.shade_device(bufs[0], bufs[1], d_colors, (255, 255, 255), edl),
                                      args.reps))
                per_pixel = None if world is not None else \
                    1e6 * float(np.median(stage[1])) / (n * len(views) * (2 * point_size + 1) ** 2)
                rows.append(dict(set=name, points=n, views=len(views), radius=label, fill_ms=stage[0],
                                 splat_ms=stage[1], resolve_ms=stage[2], shade_ms=stage[3], ns_per_pixel=per_pixel,
                                 device_wall_ms=device_wall, numpy_wall_ms=numpy_wall, **ops))
                lines.append(f'{name:8s} {n:7d} {len(views):2d} {label:>6s} | {cell(stage[0])} | {cell(stage[1])} | '
                             f'{cell(stage[2])} | {cell(stage[3])} | '
                             f'{"-" if per_pixel is None else format(per_pixel, ".3f")} | {cell(device_wall, 2)} | '
                             f'{cell(numpy_wall, 1)} | {cell(ops["rasterize_device"], 2)} | '
                             f'{cell(ops["rasterize_numpy"], 1)} | {cell(ops["shade_device"], 2)} | '
                             f'{cell(ops["shade_numpy"], 1)}')
                print(lines[-1], flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            png = wall_ms(lambda: R.write_png(os.path.join(tmp, 'sheet.png'), sheet), args.reps, False)
            size = os.path.getsize(os.path.join(tmp, 'sheet.png'))
        ply = ply_yardstick(xyz, np.asarray(rgb, np.float32), inst, args.reps)
        rows.append(dict(set=name, points=n, write_png_ms=png, png_bytes=size, save_visualizations_ply_ms=ply))
        lines.append(f'{name:8s} {n:7d} write_png of the {sheet.shape[1]} x {sheet.shape[0]} sheet ({size} bytes): '
                     f'{cell(png, 1)} | save_visualizations, input PLY, numpy: {cell(ply, 1)}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
