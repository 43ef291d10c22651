"""Runs the REFERENCE's tools/test.py save_* functions (imported by path; authoring container only) on the
inputs of save_results_cases.py and records the trees they write -> tests/golden/save_results_golden.json:
per case the relative path, size and SHA-256 of every file, the files' bytes (base64) for the tiny cases, and
the exception name where the reference raises (the unmapped panoptic class).

tools/test.py imports munch, spconv-backed model code and the rest of its package at the top; none of that is
used by the four functions, so those imports are satisfied with placeholder modules.  rle_decode is the
reference's real softgroup/util/rle.py."""
import base64
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import save_results_cases as sc  # noqa: E402

REF_ROOT = '/root/reference'
REF = os.path.join(REF_ROOT, 'tools', 'test.py')


class _Placeholder(types.ModuleType):
    """a module whose every attribute exists (None): `from x import a, b` succeeds"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return None


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod            # (the functions' multiprocessing.Pool pickles by module name)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    rle = _load('ref_softgroup_rle', os.path.join(REF_ROOT, 'softgroup', 'util', 'rle.py'))
    for name in ('munch', 'tqdm', 'softgroup', 'softgroup.data', 'softgroup.evaluation', 'softgroup.model',
                 'softgroup.util'):
        if name.startswith('softgroup') or importlib.util.find_spec(name) is None:
            sys.modules[name] = _Placeholder(name)
    sys.modules['softgroup.util'].rle_decode = rle.rle_decode
    ref = _load('ref_tools_test', REF)
    assert ref.rle_decode is rle.rle_decode
    return ref


def tree(root, with_bytes):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            data = open(p, 'rb').read()
            e = dict(size=len(data), sha256=hashlib.sha256(data).hexdigest())
            if with_bytes:
                e['b64'] = base64.b64encode(data).decode()
            out[os.path.relpath(p, root).replace(os.sep, '/')] = e
    return dict(sorted(out.items()))


def run_case(ref, case, root):
    kind, args = case['kind'], case['args']
    if kind == 'pred':
        ref.save_pred_instances(root, 'pred_instance', *args)
    elif kind == 'gt':
        ref.save_gt_instances(root, 'gt_instance', *args)
    elif kind == 'panoptic':
        ref.save_panoptic(root, 'panoptic', *args)
    else:
        scan_ids, named = args
        for name, arrs in named.items():
            ref.save_npy(root, name, scan_ids, arrs)


def expected_files(case):
    kind, args = case['kind'], case['args']
    if kind == 'pred':
        return sum(1 + len(insts) for insts in args[1])
    if kind == 'npy':
        return len(args[0]) * len(args[1])
    return len(args[0])


def main():
    ref = load_reference()
    gold = {}
    for name, case in sc.cases().items():
        with tempfile.TemporaryDirectory() as root:
            raised = None
            try:
                run_case(ref, case, root)
            except KeyError:
                raised = 'KeyError'
            assert raised == case.get('raises'), (name, raised)
            entry = dict(files=tree(root, case['tiny']))
            if raised:
                entry = dict(raises=raised)
            else:
                assert len(entry['files']) == expected_files(case), (name, len(entry['files']))
            gold[name] = entry
    path = os.path.join(HERE, 'save_results_golden.json')
    json.dump(gold, open(path, 'w'), indent=0, sort_keys=True)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
