"""The environment knobs the code reads are the ones INTEGRATION.md documents, and the retired ones stay
out (CPU only: the sources and the documents are read as text)."""
import glob
import os
import re

from conftest import ROOT

PKG = os.path.join(ROOT, "riemannian-interior-point-trust-region-method_amd")

# knobs of concluded A/B experiments, removed together with the code only they reached
RETIRED = [
    "RIPTRM_EIG_THREADS", "RIPTRM_EIG_SPLIT", "RIPTRM_EIG_BIS", "RIPTRM_EIG_TRI", "RIPTRM_TRI_MIN", "RIPTRM_TRI_RW",
    "RIPTRM_TRI_SPREAD", "RIPTRM_TRI_SLEEP", "RIPTRM_TRI_REFL", "RIPTRM_TRI_REFL_E", "RIPTRM_CG_LDS", "RIPTRM_CG_WAVE",
    "RIPTRM_SUP_DYNAMIC",
]
# RIPTRM_BIG_EIG stays with two states; these values selected the retired rocSOLVER variants
RETIRED_BIG_EIG_VALUES = ("j", "dj", "s")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc_files():
    return sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")))


def _package_files():
    return sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))


def _script_files():
    return sorted(p for p in glob.glob(os.path.join(ROOT, "scripts", "*")) if os.path.isfile(p))


def knobs_in_code():
    names = set()
    for p in _csrc_files():
        names.update(re.findall(r'\bgetenv(?:_is)?\(\s*"(RIPTRM_[A-Z0-9_]+)"', _read(p)))
    for p in _package_files():
        names.update(re.findall(r'os\.environ(?:\.\w+)?\s*[\(\[]\s*"(RIPTRM_[A-Z0-9_]+)"', _read(p)))
    return names


def knobs_in_integration_md():
    """The first column of INTEGRATION.md's knob table: rows of the form | `RIPTRM_NAME` | effect |."""
    return set(re.findall(r"^\|\s*`(RIPTRM_[A-Z0-9_]+)`\s*\|", _read(os.path.join(ROOT, "INTEGRATION.md")), re.M))


def test_code_knobs_are_the_documented_ones():
    code, doc = knobs_in_code(), knobs_in_integration_md()
    assert len(code) >= 10, sorted(code)   # the patterns still find the reads
    assert code == doc, {"undocumented": sorted(code - doc), "documented but not read": sorted(doc - code)}


def test_retired_knobs_stay_out():
    assert not set(RETIRED) & knobs_in_integration_md()
    pat = re.compile(r"(?<![A-Z0-9_])(?:" + "|".join(RETIRED) + r")(?![A-Z0-9_])")
    val = re.compile(r"RIPTRM_BIG_EIG=(?:" + "|".join(RETIRED_BIG_EIG_VALUES) + r")\b")
    hits = []
    for p in _csrc_files() + _package_files() + _script_files():
        text = _read(p)
        for m in list(pat.finditer(text)) + list(val.finditer(text)):
            hits.append((os.path.relpath(p, ROOT), text.count("\n", 0, m.start()) + 1, m.group(0)))
    assert not hits, hits
