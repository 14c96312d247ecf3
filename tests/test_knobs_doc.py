"""The runtime knobs and their documentation stay in step: every WR_*
environment variable the library or winmad_rt reads has a place in
INTEGRATION.md's "Runtime configuration" table, and every WR_* variable the
table's first column names is read somewhere.  And every knob the table
promises the same answers for is named in the GPU suite: "the cost of an
untested path in a drop-in library is an untested answer" (VERDICT.md)."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "winmad-s-raytracer-v1.0_amd")
NAME = r"(WR_[A-Z0-9_]+)"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _native_reads():
    names = set()
    for pat in ("*.hip", "*.cpp", "*.h"):
        for p in glob.glob(os.path.join(PKG, "csrc", pat)):
            names |= set(re.findall(r'getenv\(\s*"' + NAME + '"', _read(p)))
    return names


def _python_reads(paths):
    names = set()
    for p in paths:
        names |= set(re.findall(r'(?:environ(?:\.get|\.setdefault|\.pop)?|getenv)\s*[\[(]\s*["\']' + NAME, _read(p)))
    return names


def _section():
    text = _read(os.path.join(REPO, "INTEGRATION.md"))
    start = text.index("## Runtime configuration")
    end = text.find("\n## ", start + 1)
    return text[start:end if end > 0 else len(text)]


def _first_column():
    rows = [ln for ln in _section().splitlines() if ln.startswith("|") and not ln.startswith("|---")]
    return set(re.findall(NAME, " ".join(ln.split("|")[1] for ln in rows[1:])))


def test_every_knob_read_is_documented():
    read = _native_reads() | _python_reads(glob.glob(os.path.join(PKG, "winmad_rt", "*.py")))
    assert len(read) > 30, read  # the patterns still find the reads
    documented = set(re.findall(NAME, _section()))
    assert read <= documented, sorted(read - documented)


def test_every_documented_knob_is_read():
    read = _native_reads() | _python_reads(glob.glob(os.path.join(PKG, "winmad_rt", "*.py")) +
                                           [os.path.join(REPO, "bench.py")])
    named = _first_column()
    assert len(named) > 30, named
    assert named <= read, sorted(named - read)


SAME = re.compile(r"same (answers|merges|rays)", re.I)
# rows that promise the same result and cannot be tested in-process on one device:
# WR_EVENT_SYSTEM_FENCE is read once per process, at the first event made (a test would have to start a
# process); WR_MULTI_REDUCE takes several distinct devices (tests/test_gpu_dist.py's ground)
NOT_IN_PROCESS = {"WR_EVENT_SYSTEM_FENCE", "WR_MULTI_REDUCE"}


def _same_answer_knobs():
    """The first-column WR_* names of every table row whose effect text
    promises the same answers / merges / rays."""
    rows = [ln for ln in _section().splitlines() if ln.startswith("|") and not ln.startswith("|---")]
    names = set()
    for ln in rows[1:]:
        cols = ln.split("|")
        if SAME.search(cols[3]):
            names |= set(re.findall(NAME, cols[1]))
    return names


def test_every_same_answers_knob_is_named_in_a_gpu_test():
    """A knob documented as changing nothing but speed is set by at least one
    tests/test_gpu*.py: its path's answers are compared with a reference
    somewhere.  (Named, as a quoted string: what each test does with it is the
    reviewer's to read.)"""
    knobs = _same_answer_knobs()
    # the rows the promise is known to stand in: the pattern still finds them
    assert {"WR_TIE_WAVE_MAX", "WR_SCAN_WAVES", "WR_WALK_WAVE", "WR_VCM_CELL", "WR_TRACE_NO_CUT", "WR_SHADE_GRID",
            "WR_RESOLVE_GRID", "WR_ISSUE_THREADS", "WR_TRACE_WAVES_PER_CU", "WR_FAST_WAVES_PER_CU", "WR_PAIR_RECORD",
            "WR_QUEUE_SLAB", "WR_RESOLVE_LIST", "WR_BVH_WIDE", "WR_BVH_WIDE_LAT", "WR_BVH_TOP", "WR_BVH_TOP_WG",
            "WR_BDPT_OVERLAP"} <= knobs, sorted(knobs)
    assert not (knobs & NOT_IN_PROCESS), sorted(knobs & NOT_IN_PROCESS)  # (their rows promise no such thing)
    text = "".join(_read(p) for p in sorted(glob.glob(os.path.join(REPO, "tests", "test_gpu*.py"))))
    quoted = set(re.findall(r'["\']' + NAME + r'["\']', text))
    assert knobs <= quoted, sorted(knobs - quoted)
