"""CPU-side checks of the contribution-plot surface: the C ABI declares
ocm_contrib_f32 / _f64 and the binding lists them with the header's argument
count; the estimator has decision_function / contributions, and contributions
rejects a bad class or grouping before any device work."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ocm.h")


def header_argcount(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*int\s+" + name + r"\s*\((.*?)\)\s*;", txt, re.M | re.S)
    assert m, f"include/ocm.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ["ocm_contrib_f32", "ocm_contrib_f64"])
def test_header_and_binding_declare_contrib(name):
    from ocm import _lib

    n = header_argcount(name)
    assert n == 20
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_i32 and len(args) == n
    assert _lib.ABI_VERSION == 12


def test_estimator_has_the_methods():
    from utils import SIMCA

    assert callable(getattr(SIMCA, "decision_function", None))
    assert callable(getattr(SIMCA, "contributions", None))


def _stub(classes):
    """A fitted-state stub: no device, no arrays (the argument checks come first)."""
    from utils import SIMCA

    est = SIMCA(n_components=2, model_class=list(classes), verbose=False)
    est._model = {c: {"T2_limit": 1.0, "Q_limit": 1.0, "D_limit": 1.0} for c in classes}
    est._fits = {c: object() for c in classes}
    est._out_dtype = np.float32
    est._sharded = False
    return est


def test_contributions_argument_errors():
    X = np.zeros((6, 8), dtype=np.float32)
    one, two = _stub([0]), _stub([0, 1])
    with pytest.raises(ValueError, match="unknown class"):
        one.contributions(X, cls=7)
    with pytest.raises(ValueError, match="classes"):
        two.contributions(X)
    with pytest.raises(ValueError, match="rows"):
        one.contributions(X, groups=np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        one.contributions(X, groups=np.array([0, 1, 2, 3, 4, 0]))
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        one.contributions(X, groups=np.array([0, 1, -1, 0, 0, 0]))
    with pytest.raises(ValueError, match="groups="):
        one.contributions(X, groups="accepted")
