"""CPU, source text only: the library's environment knobs are the two tables of csrc/dev.cpp (OPTION_TABLE: the per-ctx
options, LH_<NAME> defaults; KNOB_TABLE: everything process-wide), and every LH_* variable the tests, bench.py, the live
tools and the documents set is read by someone - a table, or the Python side itself.  A script that sets a knob the
library no longer reads measures nothing and says nothing (tools/history/README.md)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-lasso_amd", "csrc")
TABLE_FILE = os.path.join(CSRC, "dev.cpp")


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def table_names():
    """(the options' variables, the knob table's variables in row order, the Knob enum's names in order)"""
    text = read(TABLE_FILE)
    options = {"LH_" + n.upper() for n in re.findall(r'\{"(\w+)", &Options::\w+', text)}
    knobs = re.findall(r'\{"(LH_\w+)", (?:INT|REAL|WORD|PATH)\b', text[text.index("KNOB_TABLE[] = {"):])
    enum = read(os.path.join(CSRC, "dev.hpp"))
    enum = enum[enum.index("enum class Knob {"):]
    enum = re.findall(r"\b([A-Z][A-Z0-9_]*)\b", re.sub(r"//[^\n]*", "", enum[enum.index("{") + 1:enum.index("}")]))
    return options, knobs, enum[:-1]  # (the last enumerator is COUNT)


def python_reads():
    """LH_* names the Python side reads from os.environ itself (the package, bench.py, the tools, the suite's conftest)"""
    files = (glob.glob(os.path.join(ROOT, "halo2-lasso_amd", "*.py")) + [os.path.join(ROOT, "bench.py")] +
             glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "tests", "conftest.py")])
    names = set()
    for f in files:
        text = read(f)
        names |= set(re.findall(r'os\.environ(?:\.get)?\s*[\[(]\s*"(LH_\w+)"', text))
        names |= set(re.findall(r'"(LH_\w+)"\s+(?:not\s+)?in\s+os\.environ', text))
    return names


def names_set():
    """{name: [files]} of every LH_* variable set in an environment: env dict keys, NAME= (keyword arguments, shell lines,
    documents), setenv("NAME")"""
    files = (glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py")] +
             glob.glob(os.path.join(ROOT, "tools", "*.sh")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) +
             [os.path.join(ROOT, d) for d in ("README.md", "INTEGRATION.md", "DESIGN.md")])
    found = {}
    for f in files:
        text = read(f)
        names = set(re.findall(r'\b(LH_[A-Z0-9_]+)=(?!=)', text))                # NAME=value, dict(os.environ, NAME=...)
        names |= set(re.findall(r'"(LH_[A-Z0-9_]+)"\s*:', text))                  # {"NAME": value}
        names |= set(re.findall(r'\[\s*"(LH_[A-Z0-9_]+)"\s*\]\s*=(?!=)', text))  # env["NAME"] = value
        names |= set(re.findall(r'setenv\(\s*"(LH_[A-Z0-9_]+)"', text))           # monkeypatch.setenv("NAME", ...)
        for n in names:
            found.setdefault(n, []).append(os.path.relpath(f, ROOT))
    return found


def test_only_the_knob_table_reads_the_environment():
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if path == TABLE_FILE or not path.endswith((".cpp", ".hip", ".hpp", ".cuh", ".inc")):
            continue
        for arg in re.findall(r'\bgetenv\s*\(\s*([^)]*)\)', read(path)):
            # (jit.cpp's default cache directory follows XDG_CACHE_HOME / HOME: not the library's knobs)
            if arg.strip() not in ('"XDG_CACHE_HOME"', '"HOME"'):
                offenders.append("%s: getenv(%s)" % (os.path.basename(path), arg))
    assert not offenders, "environment reads outside dev.cpp's tables: %s" % offenders


def test_knob_table_rows_follow_the_enum():
    """knob(Knob::X) reads row X of KNOB_TABLE: row i must be the variable LH_<name of enumerator i>"""
    options, knobs, enum = table_names()
    assert len(options) >= 10 and len(knobs) >= 30, "the tables of dev.cpp were not found"
    assert knobs == ["LH_" + e for e in enum]
    assert not options & set(knobs), "a variable in both tables"


def test_every_variable_set_is_read():
    options, knobs, _ = table_names()
    known = options | set(knobs) | python_reads()
    unread = {n: files for n, files in names_set().items() if n not in known}
    assert not unread, "LH_* variables set but read by no one (retired knobs? move the script to tools/history/): %s" % unread
