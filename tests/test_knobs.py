"""The table of environment variables (ffcnn_amd/csrc/ffgpu_knobs.hpp) as ffgpu_knobs_text reports it, without a GPU: the table's shape, the parse
rule of every kind, the defaults that tests and tools repeat, and that the code, the tests and tools, and INTEGRATION.md section 6 name the same
variables -- no read outside the table, no name outside it that the library would ignore, no table entry the document leaves out."""
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
KINDS = {"INT", "ON", "SET", "TEXT"}
CLASSES = {"product", "tuning", "test", "lab"}
TOKEN = re.compile(r"FFGPU_[A-Z0-9_]*[A-Z0-9]_?")         # (a trailing underscore: a family spelt by its prefix, as in a comment's FFGPU_K_* or a "FFGPU_DW_" + name)
# the values every rule is asked about (None: the variable is not set), and what each kind makes of them -- written down from the rules in the
# header of ffgpu_knobs.hpp, not asked of the library.  atoi("abc") = atoi("") = 0.
VALUES = [None, "", "0", "1", "7", "-3", "abc"]


def expect(kind, default):
    if kind == "INT":              # unset or empty: the default ("default" where the reader computes it); otherwise atoi
        d = "default" if default == "computed" else str(default)
        return [d, d, "0", "1", "7", "-3", "0"]
    if kind == "ON":               # atoi != 0
        return ["0", "0", "0", "1", "1", "1", "0"]
    if kind == "SET":              # present at all, an empty value included
        return ["0", "1", "1", "1", "1", "1", "1"]
    return ["unset"] + ["set"] * 6   # TEXT: the string itself; the report says whether there is one


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module")
def table(capi):
    return {k["name"]: k for k in capi.knobs()}


def test_table_shape(capi, table):
    rows = capi.knobs()
    assert len(rows) == len(table) > 90, "names are unique"
    for k in rows:
        assert re.fullmatch(r"(FFGPU|FFCNN)_[A-Z0-9_]*[A-Z0-9]", k["name"]), k
        assert k["kind"] in KINDS and k["cls"] in CLASSES and k["text"].strip(), k
        assert (k["default"] is None) == (k["kind"] == "TEXT"), k
        assert k["default"] != "computed" or k["kind"] == "INT", k
    assert "FFCNN_COMPAT_V6" in table
    assert {n for n, k in table.items() if k["default"] == "computed"} == {"FFGPU_IRBW_GWAVES", "FFGPU_THIN_BAND", "FFGPU_FRONT_BAND", "FFGPU_NV12_FRONT"}
    # the report is the header's table; what only a lab build reads is not in the product's (tests/test_cabi_exports.py looks at the library's
    # bytes), and those three are the TEXT knobs
    assert set(table) <= source_names()
    if b" DIAG " not in capi.lib().ffgpu_build_info():
        assert source_names() - set(table) == {"FFGPU_DBG_SKIP", "FFGPU_DBG_KEEP", "FFGPU_PWXT_TRACE"}


def test_parse_rules_by_kind(capi, table, monkeypatch):
    sets = [n for n, k in table.items() if k["kind"] == "SET"]
    assert {"FFGPU_NO_U8_FRONT", "FFGPU_VERBOSE"} <= set(sets)
    texts = [n for n, k in table.items() if k["kind"] == "TEXT"]                 # (none in a product build: the rule is checked where there is one)
    assert (table["FFGPU_IRBW_X3"]["kind"], table["FFGPU_PWXT_NT"]["kind"], table["FFGPU_THIN_BAND"]["kind"], table["FFGPU_NO_GRAPH"]["kind"]) == ("INT", "INT", "INT", "ON")
    assert (table["FFGPU_IRBW_X3"]["default"], table["FFGPU_PWXT_NT"]["default"], table["FFGPU_THIN_BAND"]["default"]) == (30, -1, "computed")
    for name in ["FFGPU_IRBW_X3", "FFGPU_PWXT_NT", "FFGPU_THIN_BAND", "FFGPU_NO_GRAPH", "FFCNN_COMPAT_V6"] + sets + texts:
        want = expect(table[name]["kind"], table[name]["default"])
        for v, w in zip(VALUES, want):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
            got = {k["name"]: k["value"] for k in capi.knobs()}[name]
            assert got == w, (name, v, got, w)
        monkeypatch.delenv(name, raising=False)
    # Today's behaviour, pinned and not endorsed: FFGPU_NO_U8_FRONT is a "set at all" switch, so =0 switches the staged path ON, while the =0 of
    # an INT or ON switch such as FFGPU_NO_FRONT switches nothing.
    monkeypatch.setenv("FFGPU_NO_U8_FRONT", "0")
    monkeypatch.setenv("FFGPU_NO_FRONT", "0")
    now = {k["name"]: k["value"] for k in capi.knobs()}
    assert now["FFGPU_NO_U8_FRONT"] == "1" and now["FFGPU_NO_FRONT"] == "0"


def test_defaults_repeated_elsewhere(table):
    """the few defaults that tests, tools and the document state as a literal next to the name"""
    assert table["FFGPU_IRBW_X3"]["default"] == 30               # tests/test_irb_choice.py ("which the default 30 has not"), INTEGRATION.md section 6
    assert "FFGPU_IRBW_X3, which the default 30 has not" in open(os.path.join(ROOT, "tests", "test_irb_choice.py")).read()
    assert table["FFGPU_IRBW_XCD"]["default"] == 3               # "default 3"
    # os.environ.get("NAME", "<number>") in a tool or test repeats the library's default
    seen = 0
    for path in text_files("tests", "tools"):
        for name, lit in re.findall(r"environ\.get\(\"(FFGPU_[A-Z0-9_]+)\",\s*\"(-?\d+)\"\)", open(path, errors="replace").read()):
            assert table[name]["default"] == int(lit), (path, name, lit)
            seen += 1
    assert seen >= 1                                             # (tools/pw_gemm_bench.py: FFGPU_PWG_NARROW)


def text_files(*tops):
    for top in tops:
        for base, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d not in ("__pycache__", "lib", "bin", "build")]
            for f in files:
                if f.endswith((".py", ".sh", ".md", ".txt", ".json", ".hip", ".c", ".cc", ".h", ".hpp")):
                    yield os.path.join(base, f)


def source_names():
    """the names of the table as the header spells them, the rows of lab builds included"""
    return set(re.findall(r"^\s*X\(\w+,\s*\"(\w+)\",", open(os.path.join(CSRC, "ffgpu_knobs.hpp")).read(), flags=re.M))


def section6():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    return txt[txt.index("\n## 6. "):txt.index("\n## 7. ")]


def test_no_stray_reads():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".inc", ".hpp", ".h")) and f != "ffgpu_knobs.hpp":
            assert "getenv" not in open(os.path.join(CSRC, f)).read(), f


def test_names_used_outside_the_library_are_read_by_it():
    """an FFGPU_* token in the tests, the tools, bench.py, the Python package or section 6 is a variable of the table, or an identifier that a
    public header or a header of the device library defines: nothing sets or documents a variable the library does not read"""
    defined = set()
    headers = [os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")]
    headers += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp"))]
    for h in headers:
        txt = open(h).read()
        defined |= set(re.findall(r"#\s*define\s+(FFGPU_[A-Z0-9_]+)", txt)) | set(re.findall(r"^\s*(FFGPU_[A-Z0-9_]+)\s*=", txt, flags=re.M))
    used = {}
    paths = list(text_files("tests", "tools")) + [os.path.join(ROOT, "bench.py")]
    paths += [os.path.join(ROOT, "ffcnn_amd", f) for f in os.listdir(os.path.join(ROOT, "ffcnn_amd")) if f.endswith(".py")]
    for path in paths:
        for t in TOKEN.findall(open(path, errors="replace").read()):
            used.setdefault(t, os.path.relpath(path, ROOT))
    for t in TOKEN.findall(section6()):
        used.setdefault(t, "INTEGRATION.md section 6")
    known = source_names() | defined
    stray = {t: where for t, where in used.items() if not (any(n.startswith(t) for n in known) if t.endswith("_") else t in known)}
    assert not stray, stray
    assert not [t for t in TOKEN.findall(section6()) if t.endswith("_")], "section 6 writes every name out"


def test_section6_names_every_knob(table):
    doc = set(re.findall(r"(?:FFGPU|FFCNN)_[A-Z0-9_]*[A-Z0-9]", section6()))
    missing = [n for n in sorted(source_names() | set(table)) if n not in doc]
    assert not missing, missing
    stale = [n for n, k in table.items() if k["cls"] != "product" and k["text"] not in section6()]      # (the product switches have their prose)
    assert not stale, stale
