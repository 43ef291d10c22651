"""The object table of a test run's saved instances: per instance its population, boxes (axis-aligned and oriented in
yaw), centroid, second moments, mean colour and semantic vote (softgroup_amd.util.describe_instances), as JSON.

    python tools/objects.py --prediction_path results --room_name scene0011_00 --out-dir objects
    python tools/objects.py --prediction_path results --all-rooms --out-dir objects [--yaw-steps 90] [--refine 0]

Reads <prediction_path>/pred_instance/<scan>.txt with its masks and <prediction_path>/coords/<scan>.npy; colours
(<prediction_path>/colors) and the semantic vote (<prediction_path>/semantic_pred, with --n-classes) are added where the
arrays exist.  Writes <out-dir>/<scan>.objects.json (softgroup_amd.util.load_objects reads it back).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd.util import describe_instances, load_pred_instances, save_objects  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--prediction_path', default='./results', help="the test run's --out directory")
    ap.add_argument('--room_name', default='scene0011_00', help='scan (file stem under <prediction_path>/coords)')
    ap.add_argument('--all-rooms', action='store_true', help='every room of the prediction path')
    ap.add_argument('--out-dir', required=True, help='directory of the <scan>.objects.json files')
    ap.add_argument('--yaw-steps', type=int, default=90, help='directions of the yaw sweep over [0, 90) degrees')
    ap.add_argument('--refine', type=int, default=0, help='refinement angles on either side of the coarse winner')
    ap.add_argument('--n-classes', type=int, help='classes of the semantic vote (without it: no vote)')
    ap.add_argument('--backend', default='auto', choices=('auto', 'device', 'numpy'))
    return ap.parse_args(argv)


def rooms_of(prediction_path):
    coords = os.path.join(prediction_path, 'coords')
    return sorted(f[:-4] for f in os.listdir(coords) if f.endswith('.npy')) if os.path.isdir(coords) else []


def _array(prediction_path, directory, room):
    path = os.path.join(prediction_path, directory, room + '.npy')
    return np.load(path) if os.path.exists(path) else None


def describe_room(opt, room):
    coords = _array(opt.prediction_path, 'coords', room)
    if coords is None:
        sys.exit(f'{opt.prediction_path}/coords/{room}.npy not found')
    insts = load_pred_instances(os.path.join(opt.prediction_path, 'pred_instance'), room, backend=opt.backend)
    semantic = _array(opt.prediction_path, 'semantic_pred', room) if opt.n_classes is not None else None
    table = describe_instances(insts, coords, _array(opt.prediction_path, 'colors', room), semantic,
                               opt.n_classes if semantic is not None else None, opt.yaw_steps, opt.refine, opt.backend)
    os.makedirs(opt.out_dir, exist_ok=True)
    path = os.path.join(opt.out_dir, room + '.objects.json')
    save_objects(path, table)
    return path, len(insts)


def main(argv=None):
    opt = parse_args(argv)
    rooms = rooms_of(opt.prediction_path) if opt.all_rooms else [opt.room_name]
    if not rooms:
        sys.exit(f'no rooms under {opt.prediction_path}/coords')
    for room in rooms:
        path, n = describe_room(opt, room)
        print(f'{path}: {n} objects')


if __name__ == '__main__':
    main()
