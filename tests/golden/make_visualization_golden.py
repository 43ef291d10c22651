"""Runs the REFERENCE's tools/visualization.py (imported by path; authoring container only -- the module needs
only numpy) on the trees of visualization_cases.py and records, per case and task, what ``get_coords_color`` and
``write_ply`` produce -> tests/golden/visualization_golden.json:

    size, sha256     of the PLY file; b64: its bytes, for the tiny cases
    xyz_sha256       of the returned xyz (float32 bytes)
    rgb_dtype, rgb_sha256   of the returned rgb
    printed_sha256   of the colours write_ply prints, int64 [m, 3]
    raises           the exception name where the reference raises

plus, under "write_ply", the bytes of two direct write_ply calls (faces; colors=None).  A case's declared
``errors`` must be what the reference raises, and it may fail elsewhere only where the case says ``instead``."""
import argparse
import base64
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import visualization_cases as vc  # noqa: E402

REF = '/root/reference/tools/visualization.py'


def load_reference():
    spec = importlib.util.spec_from_file_location('ref_tools_visualization', REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def direct_calls():
    """arguments of the two direct write_ply calls"""
    rng = np.random.default_rng(77)
    verts = rng.standard_normal((9, 3)).astype(np.float32)
    colors = rng.uniform(0, 1, size=(9, 3))
    faces = np.array([[0, 1, 2], [2, 3, 4], [8, 7, 6]], dtype=np.int64)
    return dict(faces=(verts, colors, faces), no_colors=(verts.astype(np.float64) * 1000, None, None))


def run(ref, case, task, root, ply):
    opt = argparse.Namespace(prediction_path=root, room_name=case['room'], task=task)
    with contextlib.redirect_stdout(io.StringIO()):
        xyz, rgb = ref.get_coords_color(opt)
    colors = rgb / 255                                       # (the reference's __main__)
    ref.write_ply(xyz[:, :3], colors, None, ply)
    data = open(ply, 'rb').read()
    printed = np.array([[int(c * 255) for c in row] for row in colors], dtype=np.int64).reshape(-1, 3)
    e = dict(size=len(data), sha256=hashlib.sha256(data).hexdigest(), xyz_sha256=sha(xyz), rgb_dtype=str(rgb.dtype),
             rgb_sha256=sha(rgb), printed_sha256=sha(printed))
    if case['tiny']:
        e['b64'] = base64.b64encode(data).decode()
    return e


def main():
    ref = load_reference()
    gold = {}
    for name, case in vc.cases().items():
        vc.check_distinct(case)
        gold[name] = {}
        with tempfile.TemporaryDirectory() as root:
            vc.write_tree(case, root)
            for task in vc.TASKS:
                try:
                    entry = run(ref, case, task, root, os.path.join(root, 'out.ply'))
                except Exception as e:  # noqa: BLE001
                    entry = dict(raises=type(e).__name__)
                    assert case['errors'].get(task) == entry['raises'] or task in case['instead'], (name, task, repr(e))
                else:
                    assert task not in case['errors'] and task not in case['instead'], (name, task)
                gold[name][task] = entry
    gold['write_ply'] = {}
    with tempfile.TemporaryDirectory() as root:
        for name, args in direct_calls().items():
            p = os.path.join(root, name + '.ply')
            ref.write_ply(*args, p)
            gold['write_ply'][name] = base64.b64encode(open(p, 'rb').read()).decode()
    path = os.path.join(HERE, 'visualization_golden.json')
    json.dump(gold, open(path, 'w'), indent=0, sort_keys=True)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
