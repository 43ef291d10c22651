"""DESIGN.md section 8 lists exactly the SG_* environment variables that the package reads: every
getenv("SG_...") in softgroup_amd/csrc and every os.environ read of an SG_ name in the Python package
has a row in the table, and every row is still read.  The second list of the section (names that only
bench.py, tests/, tools/ or oracle/ read) is checked one way: each entry occurs under those paths."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'softgroup_amd')
NAME = r'SG_[A-Z0-9_]+'


def _read(path):
    with open(path, errors='replace') as f:
        return f.read()


def _names_read_by_package():
    names = set()
    csrc = os.path.join(PKG, 'csrc')
    for f in sorted(os.listdir(csrc)):
        names.update(re.findall(r'getenv\("(%s)"\)' % NAME, _read(os.path.join(csrc, f))))
    for f in glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True):
        names.update(re.findall(r'''os\.environ(?:\.get\(|\[)\s*['"](%s)['"]''' % NAME, _read(f)))
    return names


def _section8():
    txt = _read(os.path.join(ROOT, 'DESIGN.md'))
    sec = txt[txt.index('\n## 8. '):]
    sec = sec[:sec.index('\n## ', 1)]
    main, _, second = sec.partition('\n### ')
    first_column = r'^\|\s*`(%s)`\s*\|' % NAME
    return set(re.findall(first_column, main, flags=re.M)), set(re.findall(first_column, second, flags=re.M))


def test_design_section_8_lists_the_knobs_the_package_reads():
    read = _names_read_by_package()
    listed, _ = _section8()
    assert len(read) > 20
    print('read but not listed:', sorted(read - listed))
    print('listed but not read:', sorted(listed - read))
    assert read == listed


def test_second_list_names_occur_where_it_says():
    listed, second = _section8()
    assert second and not (second & listed)
    files = [os.path.join(ROOT, 'bench.py')]
    for d in ('tests', 'tools', 'oracle'):
        files += [f for f in glob.glob(os.path.join(ROOT, d, '**', '*'), recursive=True)
                  if os.path.isfile(f) and f.endswith(('.py', '.sh')) and os.path.abspath(f) != os.path.abspath(__file__)]
    text = '\n'.join(_read(f) for f in files)
    missing = sorted(n for n in second if not re.search(r'\b%s\b' % n, text))
    print('listed but read nowhere:', missing)
    assert not missing
