"""Cost of reading raw point-cloud text (softgroup_amd.ops.text.parse_table, csrc/cloud_io.hip) on files the tool
writes itself from a seed:

  s3dis     1 M rows, '%.3f %.3f %.3f %d %d %d'                    (an S3DIS room)
  stpls3d   600 k rows x 8, '%.6f', comma separated                (an STPLS3D tile)
  savetxt   150 k x 6 in np.savetxt's default '%.18e'
  ply       the vertex lines of a 150 k-vertex ASCII PLY written by softgroup_amd.util.write_ply

Reported per file, all in the same run, each the median of --reps runs after a warm-up (min .. max in brackets), ms:
  h2d          copy of the text from pinned memory to the device, HIP events
  count/parse  sg_text_table_count / sg_text_table_parse on text already on the device, HIP events
  device       parse_table(backend='device') from bytes in memory to a numpy array, wall
  numpy        parse_table_numpy (the definition), wall
  loadtxt      np.loadtxt, wall
  pandas       pandas.read_csv, wall (when importable)
Before anything is timed the device result must equal the definition's, byte for byte.

    python tools/cloud_io_bench.py [--reps 5] [--scale 1.0] [--out profiles/cloud_io_bench.txt]
"""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd.ops import text as T  # noqa: E402
from softgroup_amd.util import write_ply  # noqa: E402


def make_files(scale):
    rng = np.random.default_rng(7)
    files = []
    n = int(1000000 * scale)
    xyz = rng.uniform(-20, 20, size=(n, 3))
    rgb = rng.integers(0, 256, size=(n, 3))
    buf = io.BytesIO()
    np.savetxt(buf, np.concatenate([xyz, rgb], 1), fmt='%.3f %.3f %.3f %d %d %d')
    files.append(('s3dis', buf.getvalue(), dict(cols=6), {}))
    n = int(600000 * scale)
    buf = io.BytesIO()
    np.savetxt(buf, rng.uniform(-250, 250, size=(n, 8)), fmt='%.6f', delimiter=',')
    files.append(('stpls3d', buf.getvalue(), dict(cols=8, delimiter=','), dict(delimiter=',')))
    n = int(150000 * scale)
    buf = io.BytesIO()
    np.savetxt(buf, rng.uniform(-20, 20, size=(n, 6)))
    files.append(('savetxt', buf.getvalue(), dict(cols=6), {}))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'cloud.ply')
        write_ply(rng.uniform(-5, 5, size=(n, 3)).astype(np.float32), rng.uniform(0, 1, size=(n, 3)), None, path,
                  backend='numpy')
        raw = open(path, 'rb').read()
    body = raw[raw.index(b'end_header\n') + 11:]
    files.append(('ply', body, dict(cols=6), {}))
    return files


def stat(samples):
    s = sorted(samples)
    return '%.1f [%.1f .. %.1f]' % (s[len(s) // 2], s[0], s[-1])


def wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return stat(out)


def events(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cloud_io_bench.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'cloud_io_bench needs a GPU'
    try:
        import pandas
    except ImportError:
        pandas = None
    lines = [f'# tools/cloud_io_bench.py --reps {args.reps} --scale {args.scale}  ({torch.cuda.get_device_name(0)}); ms, '
             'median [min .. max]; device = parse_table(backend=\'device\') from bytes in memory to a numpy array',
             'file     rows cols     bytes declined | h2d | count | parse | device | numpy | loadtxt | pandas']
    for name, data, kw, np_kw in make_files(args.scale):
        ref, ref_lines = T.parse_table_numpy(data, return_lines=True, **kw)
        info = {}
        got, got_lines = T.parse_table(data, backend='device', return_lines=True, info=info, **kw)
        assert got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
        assert np.array_equal(got_lines, ref_lines), name
        n = len(data)
        pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        pinned.numpy()[:] = np.frombuffer(data, dtype=np.uint8)
        dev = torch.empty(n, dtype=torch.uint8, device='cuda')
        delim = T._delimiter_arg(kw.get('delimiter'))
        rows, cols = ref.shape
        values = torch.empty((rows, cols), dtype=torch.float64, device='cuda')
        status = torch.empty(rows, dtype=torch.uint8, device='cuda')
        line = torch.empty(rows, dtype=torch.int32, device='cuda')
        t_h2d = events(lambda: dev.copy_(pinned, non_blocking=True), args.reps)
        t_count = events(lambda: T.table_count_device(dev), args.reps)
        t_parse = events(lambda: T.table_parse_device(dev, cols, rows, delim, values=values, row_status=status,
                                                      row_line=line), args.reps)
        t_dev = wall(lambda: T.parse_table(data, backend='device', **kw), args.reps)
        t_np = wall(lambda: T.parse_table_numpy(data, **kw), args.reps)
        t_lt = wall(lambda: np.loadtxt(io.BytesIO(data), **np_kw), args.reps)
        t_pd = wall(lambda: pandas.read_csv(io.BytesIO(data), header=None, sep=np_kw.get('delimiter', ' ')).values,
                    args.reps) if pandas else 'not installed'
        lines.append(f'{name:8s} {rows:7d} {cols:2d} {n:9d} {info["declined"]:6d} | {t_h2d} | {t_count} | {t_parse} | '
                     f'{t_dev} | {t_np} | {t_lt} | {t_pd}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
