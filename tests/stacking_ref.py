"""A plain NumPy restatement of Stacking, the reference of the stacking tests; built on
predict_ref.py's tree walk (held to oracle.predict by test_predict_ref_host.py).

  level1(trees, subs, X)       the stacker's training matrix: row r is
                               Vectors.dense(models.map(_.predict(features_r)))
                               (StackingRegressor.scala:163-171)
  predict(...)                 stack.predict(Vectors.dense(models.map(_.predict(features))))
                               (StackingRegressionModel.predict, StackingRegressor.scala:233-235)
  dataset_layout(P)            what sbag_dataset_create makes of a host matrix: per-feature sorted
                               distinct values (-0.0 == 0.0), the code width, the row stride and
                               the codes with zero padding columns
"""
import numpy as np

import predict_ref as ref


def level1(trees, subs, X):
    """fp64 [N][K]: feature k of row r is tree k's prediction of row r."""
    return np.ascontiguousarray(ref.per_tree(trees, subs, X).T)


def predict(trees, subs, stack, stack_sub, X):
    """The stack tree over the level-1 matrix: its feature j is base tree stack_sub[j]."""
    return ref.per_tree([stack], [stack_sub], level1(trees, subs, X))[0]


def row_stride(F):
    return (F + 15) // 16 * 16 if F <= 64 else (F + 127) // 128 * 128


def dataset_layout(P):
    """(dict values concatenated, dict_off [F + 1], code_bytes, row_stride, codes [N][S])."""
    P = np.asarray(P, np.float64)
    N, F = P.shape
    P = np.where(P == 0.0, 0.0, P)  # canon: -0.0 -> 0.0
    dicts = [np.unique(P[:, k]) for k in range(F)]
    off = np.concatenate([[0], np.cumsum([len(d) for d in dicts])]).astype(np.int64)
    widest = max(len(d) for d in dicts)
    cb = 1 if widest <= 256 else 2 if widest <= 65536 else 4
    S = row_stride(F)
    codes = np.zeros((N, S), {1: np.uint8, 2: np.uint16, 4: np.uint32}[cb])
    for k in range(F):
        codes[:, k] = np.searchsorted(dicts[k], P[:, k])
    return np.concatenate(dicts), off, cb, S, codes
