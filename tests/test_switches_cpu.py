"""The TTV_* environment switches: tools/README.md lists every one the library and the package read, and nothing else; the reads
go through the helpers (csrc/ttv_common.h, titok_video_amd/switches.py) and nowhere else."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "titok_video_amd")
CSRC = os.path.join(PKG, "csrc")
NAME = re.compile(r'"(TTV_[A-Z0-9_]+)"')      # a string literal that is a switch name and nothing else


def _sources():
    c = [p for ext in ("*.hip", "*.inc", "*.h") for p in glob.glob(os.path.join(CSRC, ext))]
    py = glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)
    assert len(c) >= 20 and len(py) >= 20
    return c, py


def _reads_go_through_the_helpers(c, py):
    for path in c:
        n = open(path).read().count("getenv(")
        assert n == (3 if os.path.basename(path) == "ttv_common.h" else 0), path
    common = open(os.path.join(CSRC, "ttv_common.h")).read()
    for helper in ("ttv_env_flag", "ttv_env_int", "ttv_env_float"):
        body = re.search(r"static inline \w+ %s\([^)]*\) \{(.*?)\n\}" % helper, common, flags=re.S).group(1)
        assert body.count("getenv(") == 1, helper
    for path in py:
        if os.path.basename(path) != "switches.py":
            src = open(path).read()
            assert "os.environ" not in src and "getenv" not in src, path


def test_switch_table_lists_exactly_the_switches_that_are_read():
    c, py = _sources()
    _reads_go_through_the_helpers(c, py)      # so that the literals collected below are all the reads there are
    read = {}
    for path in c + py:
        for name in NAME.findall(open(path).read()):
            read.setdefault(name, set()).add(os.path.relpath(path, PKG))
    doc = open(os.path.join(ROOT, "tools", "README.md")).read()
    table = re.search(r"<!-- switch-table -->(.*?)<!-- /switch-table -->", doc, flags=re.S).group(1)
    rows = [[cell.strip() for cell in line.strip().strip("|").split("|")] for line in table.strip().splitlines()[2:]]
    assert all(len(r) == 5 and all(r) for r in rows), "name | default | values | selects | read in"
    listed = [r[0].strip("`") for r in rows]
    assert len(listed) == len(set(listed)), "a switch is listed twice"
    assert sorted(set(read) - set(listed)) == [], "read in the code, missing from the table in tools/README.md"
    assert sorted(set(listed) - set(read)) == [], "listed in tools/README.md, read nowhere"
    for name, _default, _values, _selects, where in rows:       # the table names the file that holds the read
        files = re.findall(r"`([^`]+\.(?:hip|py|h|inc))`", where)
        assert files and files[0] in read[name.strip("`")], (name, where, sorted(read[name.strip("`")]))
