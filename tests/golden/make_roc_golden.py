"""Generate tests/golden/roc.npz: scikit-learn's ROC results on fixed inputs.

    python tests/golden/make_roc_golden.py

For each named input the file holds the scores ``<name>_s``, the labels
``<name>_y`` and scikit-learn's ``roc_auc_score`` (``<name>_auc``) and
``roc_curve(drop_intermediate=False)`` (``<name>_fpr``, ``_tpr``, ``_thr``).

* normal — float64 normal draws, positives shifted, m = 400.
* ties   — scores rounded to 1/4 (heavy ties), m = 600.
* zeros  — −0.0 and +0.0 mixed with a few other values, m = 240.
* f32    — the shape of the reference's call (optim_bce_nuts.py:241,
  ``roc_auc_score(labels_true, f_all)``): float32 full distances ``f`` ≥ 0 and
  integer labels {0, 1}, the label 1 rows (the outliers) with the larger ``f``,
  m = 1000.
"""
import os

import numpy as np
from sklearn.metrics import roc_auc_score, roc_curve


def inputs():
    rng = np.random.default_rng(20240607)
    out = {}
    y = (rng.random(400) < 0.3).astype(np.int64)
    out["normal"] = (rng.standard_normal(400) + 0.8 * y, y)
    y = (rng.random(600) < 0.5).astype(np.int64)
    out["ties"] = (np.round((rng.standard_normal(600) + 0.5 * y) * 4) / 4, y)
    y = (rng.random(240) < 0.4).astype(np.int64)
    out["zeros"] = (rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.5, 2.0, 5e-324, -5e-324]), size=240), y)
    y = (rng.random(1000) < 0.2).astype(np.int64)
    f = (rng.chisquare(6, 1000) * (1.0 + 1.5 * y)).astype(np.float32)
    out["f32"] = (f, y)
    return out


def main():
    data = {}
    for name, (s, y) in inputs().items():
        fpr, tpr, thr = roc_curve(y, s, drop_intermediate=False)
        data.update({f"{name}_s": s, f"{name}_y": y, f"{name}_auc": np.float64(roc_auc_score(y, s)),
                     f"{name}_fpr": fpr, f"{name}_tpr": tpr, f"{name}_thr": thr})
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "roc.npz"), **data)


if __name__ == "__main__":
    main()
