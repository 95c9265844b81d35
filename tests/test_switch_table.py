"""The library's runtime switches live in one table (rsrgan_amd/csrc/switches.h) that one function reads.  The placement tests
compare two runs that differ in one switch: a misspelt or removed name would make both runs the same configuration and the
comparison empty.  So: every switch name the tests, the benchmark and the Python layer use is a row of the table; the table is
well-formed; nothing else in the library reads the environment; DESIGN.md lists the same rows."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rsrgan_amd", "csrc")
PREFIX = "RSRGAN_"
TOKEN = re.compile(PREFIX + r"[A-Z0-9_]+")
# read by Python code, not by the library
PYTHON_SIDE = {PREFIX + "BENCH_ENGINE", PREFIX + "FLAGS", PREFIX + "BUCKETED_ALLREDUCE"}
TEST_WORKER_PREFIX = PREFIX + "TEST_"
ROW = re.compile(r'^\s*X\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(BOOL|INT)\s*,\s*(-?\d+)\s*,\s*(ANY|MIN0|W8)\s*,\s*(handle|process|call)\s*,\s*"(.*)"\s*\)\s*\\?\s*$')


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def table_rows(text=None):
    """[(NAME, field, kind, default, clamp, scope, description)] of the X-macro list in switches.h."""
    text = _read(os.path.join(CSRC, "switches.h")) if text is None else text
    body = text.split("#define " + PREFIX + "SWITCHES(X)", 1)[1].split("// clang-format on", 1)[0]
    lines = [ln for ln in body.splitlines() if ln.strip() not in ("", "\\")]
    rows = [ROW.match(ln) for ln in lines]
    assert all(rows), "not a table row: %r" % [ln for ln, m in zip(lines, rows) if not m]
    return [m.groups() for m in rows]


def header_identifiers():
    """What include/rsrgan.h itself defines (enumerators and macros), comments left out: its prose names switches too."""
    text = re.sub(r"/\*.*?\*/", " ", _read(os.path.join(ROOT, "include", "rsrgan.h")), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = set(re.findall(r"^\s*#\s*define\s+(" + TOKEN.pattern + ")", text, re.M))
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        names.update(TOKEN.findall(body))
    return names


def python_sources():
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    files += glob.glob(os.path.join(ROOT, "rsrgan_amd", "**", "*.py"), recursive=True)
    return sorted(files)


def switch_names_used(files):
    """{name without the prefix: [files]} of every token of the switches' form that is no identifier of the C header, no variable
    of a test worker and none of the Python layer's own."""
    skip = header_identifiers() | PYTHON_SIDE
    used = {}
    for path in files:
        for tok in set(TOKEN.findall(_read(path))):
            if tok in skip or tok.startswith(TEST_WORKER_PREFIX):
                continue
            used.setdefault(tok[len(PREFIX):], []).append(os.path.relpath(path, ROOT))
    return used


def reader_sites(root=CSRC):
    """(file, line number) of every call of the C library's environment reader under csrc/."""
    sites = []
    for path in sorted(glob.glob(os.path.join(root, "*"))):
        if os.path.splitext(path)[1] in (".h", ".hip", ".cpp"):
            sites += [(os.path.basename(path), i + 1) for i, ln in enumerate(_read(path).splitlines()) if "getenv" in ln]
    return sites


def design_rows():
    """{NAME: (kind, default, scope)} of the table in DESIGN.md's section "Runtime switches"."""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## [^\n]*Runtime switches[^\n]*\n(.*?)(?=^## )", text, re.S | re.M)
    assert m, 'DESIGN.md has no section "Runtime switches"'
    rows = re.findall(r"^\| `" + PREFIX + r"(\w+)` \| (\w+) \| (-?\d+) \| (\w+) \| (.*) \|$", m.group(1), re.M)
    return rows


def test_header_parse_keeps_switches_apart():
    ids = header_identifiers()
    for n in ("OK", "ERR_NO_DEVICE", "G_LSTM", "G_BNLSTM", "D_DNN", "NET_G", "FLAG_GRAPH", "FLAG_BATCH_NORM", "D_REAL", "ADAM_STEP_D", "SEGAN_L1_LAMBDA"):
        assert PREFIX + n in ids, n
    # the header's prose speaks of a switch; names shaped like its enumerators are switches all the same
    for n in ("DPIPE", "DP_NRT", "GP_TAGS", "GP_RES", "DFOLD", "DHEAD"):
        assert PREFIX + n not in ids, n


def test_table_is_well_formed():
    rows = table_rows()
    assert len(rows) == 46
    names = [r[0] for r in rows]
    fields = [r[1] for r in rows]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert len(set(fields)) == len(fields), sorted(f for f in fields if fields.count(f) > 1)
    for name, field, kind, default, clamp, scope, doc in rows:
        assert field == name.lower(), (name, field)
        assert doc.strip(), name
        if kind == "BOOL":
            assert default in ("0", "1") and clamp == "ANY", name
    assert {r[0] for r in rows if r[5] == "handle"} == {"GPERSIST", "DPERSIST", "DFOLD", "TRAIL", "GRAPHS", "RCED_IMPLICIT", "DPIPE"}
    assert {r[0] for r in rows if r[5] == "call"} == {"GRAPH_DEBUG", "TRAIL_DBG"}


def test_every_switch_the_suite_and_the_benchmark_use_is_a_row():
    table = {r[0] for r in table_rows()}
    used = switch_names_used(python_sources())
    # the tests do flip switches: an empty scan would pass everything
    assert {"XCD_GROUPS", "GPERSIST", "DPIPE", "GP_TAGS", "DP_NRT", "CONV4", "RESIDENT_CAP"} <= set(used)
    unknown = {n: used[n] for n in used if n not in table}
    assert not unknown, "not in rsrgan_amd/csrc/switches.h: %r" % unknown


def test_the_library_reads_the_environment_in_one_place():
    assert [f for f, _ in reader_sites()] == ["switches.h"], reader_sites()


def test_design_lists_the_same_rows():
    table = {name: (kind.lower(), default, scope) for name, _, kind, default, _, scope, _ in table_rows()}
    rows = design_rows()
    assert len({r[0] for r in rows}) == len(rows)
    doc = {name: (kind, default, scope) for name, kind, default, scope, _ in rows}
    assert sorted(set(table) - set(doc)) == [] and sorted(set(doc) - set(table)) == []
    assert doc == table
    assert all(r[4].strip() for r in rows)
