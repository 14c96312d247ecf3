"""The runtime knobs and their documentation stay in step: every WR_*
environment variable the library or winmad_rt reads has a place in
INTEGRATION.md's "Runtime configuration" table, and every WR_* variable the
table's first column names is read somewhere."""
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
