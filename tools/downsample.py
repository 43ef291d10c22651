"""Thin the preprocessed S3DIS rooms before training or testing.

    python tools/downsample.py --data-dir dataset/s3dis/preprocess --ratio 0.25 --seed 0
    python tools/downsample.py --data-dir dataset/s3dis/preprocess --voxel-size 0.02 --pick center

Every ``<data-dir>/*.pth`` holds one room as a 6-tuple: four per-point arrays (coordinates, colours, semantic
labels, instance labels) followed by the room label and the scene name.  The thinned room keeps that layout and the
arrays' dtypes; only the four per-point arrays change.

  --ratio R        keep ``int(N * R)`` points drawn with ``random.Random(seed).sample`` (the draw of the reference's
                   offline step, in its unsorted order); output in ``<data-dir>_sample/``
  --voxel-size V   keep one point per occupied voxel of edge V, point order kept (the reference accepts the option
                   and stops there); output in ``<data-dir>_voxelize/``; wins over ``--ratio`` when both are given

The output file of a room is ``<scene>_inst_nostuff.pth``.  A room whose output file is already there is left alone,
so an interrupted run can simply be started again.
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from softgroup_amd.data.downsample import apply_sample, random_downsample, voxel_downsample  # noqa: E402

N_POINT_ARRAYS = 4          # leading entries of a room tuple that have one row per point


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Thin S3DIS rooms: a random subset or one point per voxel.')
    ap.add_argument('--data-dir', default='./preprocess', help='folder with the full-resolution *.pth rooms')
    ap.add_argument('--ratio', type=float, default=0.25, help='fraction of the points a random subset keeps')
    ap.add_argument('--voxel-size', type=float, default=None,
                    help='voxel edge in metres; when given, one point per voxel is kept and --ratio is unused')
    ap.add_argument('--verbose', action='store_true', help='report every room, with its point counts')
    ap.add_argument('--pick', choices=('center', 'first'), default='center',
                    help="which point stands for a voxel: the one nearest its centre, or its lowest index")
    ap.add_argument('--seed', type=int, default=None, help='seed of the random subset (omit for a fresh draw)')
    ap.add_argument('--backend', choices=('auto', 'device', 'numpy'), default='auto',
                    help='where the voxel grid is computed')
    return ap.parse_args(argv)


def choose_points(xyz, args):
    """ids of the points a room keeps"""
    if args.voxel_size is None:
        return random_downsample(len(xyz), args.ratio, seed=args.seed)
    return voxel_downsample(xyz, args.voxel_size, pick=args.pick, backend=args.backend)[0]


def main(argv=None):
    """-> the number of rooms written (rooms already thinned are not counted)"""
    args = parse_args(argv)
    by_voxel = args.voxel_size is not None
    out_dir = Path(args.data_dir + ('_voxelize' if by_voxel else '_sample'))
    out_dir.mkdir(parents=True, exist_ok=True)
    mode = f'voxel grid of {args.voxel_size} m ({args.pick})' if by_voxel else f'random subset, ratio {args.ratio}'
    print(f'{mode}: {args.data_dir} -> {out_dir}')
    n_written = 0
    for path in sorted(Path(args.data_dir).glob('*.pth')):
        room = tuple(torch.load(path, weights_only=False))
        target = out_dir / f'{room[-1]}_inst_nostuff.pth'
        if target.exists():
            if args.verbose:
                print(f'  {room[-1]}: already there, skipped')
            continue
        ids = choose_points(room[0], args)
        thinned = tuple(apply_sample(ids, *room[:N_POINT_ARRAYS])) + room[N_POINT_ARRAYS:]
        torch.save(thinned, target)
        n_written += 1
        if args.verbose:
            print(f'  {room[-1]}: {len(room[0])} -> {len(thinned[0])} points')
    print(f'{n_written} rooms written')
    return n_written


if __name__ == '__main__':
    main()
