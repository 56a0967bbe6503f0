"""ctypes bindings to libsbag.so (include/sbag.h).

The product path: every compute call goes through the HIP library.  There is
no CPU fallback; if the library is missing or fails to load, importing the
compute entry points raises.
"""
import ctypes
import weakref
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsbag.so")

SBAG_OK, SBAG_EINVAL, SBAG_EEMPTY, SBAG_EDEVICE, SBAG_ENOMEM, SBAG_EUNSUPPORTED = range(6)
IMPURITY_VARIANCE, IMPURITY_GINI = 0, 1
AGG_MEAN, AGG_MODE = 0, 1
OUT_SUM, OUT_VOTES = 2, 3  # device outputs of sbag_predict_dataset_device
RAW_VOTES, RAW_LEAF = 0, 1  # kinds of sbag_predict_raw: hard / soft voting
W_DOT, W_CLASS = 0, 1  # kinds of sbag_predict_weighted: weighted sums / class weights
COL_F64, COL_F32, COL_U8 = 0, 1, 2  # sbag_dataset_create_columns

# every symbol include/sbag.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "sbag_device_count", "sbag_ctx_create", "sbag_ctx_destroy", "sbag_last_error", "sbag_version",
    "sbag_sample", "sbag_subspace", "sbag_dataset_create", "sbag_dataset_create_csr",
    "sbag_dataset_create_columns", "sbag_dataset_synthetic",
    "sbag_dataset_info", "sbag_dataset_labels", "sbag_dataset_features", "sbag_dataset_free",
    "sbag_dataset_set_labels", "sbag_dataset_layout", "sbag_dataset_export", "sbag_dataset_import",
    "sbag_fit", "sbag_fit_booster", "sbag_forest_num_trees", "sbag_forest_tree_info", "sbag_forest_subspace",
    "sbag_forest_nodes", "sbag_forest_create", "sbag_forest_free", "sbag_forest_timing",
    "sbag_predict", "sbag_predict_dataset", "sbag_aggregate", "sbag_predict_dataset_device",
    "sbag_aggregate_device", "sbag_predict_oob", "sbag_predict_oob_permuted",
    "sbag_forest_num_classes", "sbag_forest_create_stats", "sbag_predict_raw",
    "sbag_predict_raw_dataset", "sbag_predict_oob_raw",
    "sbag_sample_boosted", "sbag_sample_boosted_stats", "sbag_fit_bag",
    "sbag_dataset_create_stacked", "sbag_predict_stacked", "sbag_predict_stacked_dataset",
    "sbag_predict_weighted", "sbag_predict_weighted_dataset", "sbag_eval_staged",
]


class SbagError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[sbag error {code}] {msg}")
        self.code = code


class IllegalArgumentException(SbagError, ValueError):
    """SBAG_EINVAL: the reference raises IllegalArgumentException (require / ParamValidators)."""


class SparkException(SbagError):
    """SBAG_EEMPTY and device failures: the reference raises SparkException."""


class SamplerParams(ctypes.Structure):
    _fields_ = [("replacement", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("sample_ratio", ctypes.c_double), ("seed", ctypes.c_int64),
                ("learner_begin", ctypes.c_int32), ("learner_end", ctypes.c_int32)]


class TreeParams(ctypes.Structure):
    _fields_ = [("max_depth", ctypes.c_int32), ("max_bins", ctypes.c_int32),
                ("min_instances_per_node", ctypes.c_int32), ("impurity", ctypes.c_int32),
                ("min_info_gain", ctypes.c_double), ("seed", ctypes.c_int64)]


# base learners' HasSeed defaults (class-name hashCode): seed of RandomForest.findSplits'
# split-finding sample
DT_SEED_REGRESSOR = 926680331     # "org.apache.spark.ml.regression.DecisionTreeRegressor"
DT_SEED_CLASSIFIER = 159147643    # "org.apache.spark.ml.classification.DecisionTreeClassifier"


class FitParams(ctypes.Structure):
    _fields_ = [("sampler", SamplerParams), ("subspace_ratio", ctypes.c_double),
                ("subspace_bug_compat", ctypes.c_int32), ("num_partitions", ctypes.c_int32),
                ("partition_offsets", ctypes.c_void_p), ("tree", TreeParams)]


class BoosterParams(ctypes.Structure):
    _fields_ = [("counts", ctypes.c_void_p), ("subspace", ctypes.c_void_p),
                ("subspace_len", ctypes.c_int32), ("num_partitions", ctypes.c_int32),
                ("partition_offsets", ctypes.c_void_p), ("tree", TreeParams)]


class Timing(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in
                ("total_ms", "sample_ms", "valuecount_ms", "bin_ms", "compact_ms", "hist_ms",
                 "split_ms", "subtract_ms")] + [
        ("hist_launches", ctypes.c_int64), ("hist_alg_bytes", ctypes.c_double),
        ("hist_entries", ctypes.c_double), ("hist_upper_bytes", ctypes.c_double),
        ("levels", ctypes.c_int64), ("partition_ms", ctypes.c_double),
        ("hist_work_bytes", ctypes.c_double), ("fix_ms", ctypes.c_double),
        ("exact_fallbacks", ctypes.c_int64), ("hist_lds_atomics", ctypes.c_double),
        ("group_ms", ctypes.c_double), ("chain_ms", ctypes.c_double),
        ("root_ms", ctypes.c_double), ("root_mfma_ops", ctypes.c_double),
        ("hist_midrun_flushes", ctypes.c_int64), ("entry_capacity", ctypes.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BoostedStats(ctypes.Structure):
    _fields_ = [("rows_zero", ctypes.c_int64), ("rows_fast", ctypes.c_int64),
                ("rows_general", ctypes.c_int64), ("fast_doubles", ctypes.c_int32),
                ("pad_", ctypes.c_int32), ("fast_ms", ctypes.c_double),
                ("general_ms", ctypes.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad_"}


# sbag_stage_stats: one record per stage of sbag_eval_staged
STAGE_DTYPE = np.dtype([("covered", "<i8"), ("correct", "<i8"), ("sum_se", "<f8"), ("sum_ae", "<f8")])

NODE_DTYPE = np.dtype([("id", "<i4"), ("left", "<i4"), ("right", "<i4"), ("feature", "<i4"),
                       ("split_bin", "<i4"), ("pad", "<i4"), ("threshold", "<f8"),
                       ("prediction", "<f8"), ("impurity", "<f8"), ("gain", "<f8")])

_lib = None


def lib():
    """Load libsbag.so; raises if it is missing (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libsbag.so not built at {LIB_PATH}: run __graft_entry__.build()")
        try:
            # PyTorch-ROCm ships its own HIP runtime under the same soname
            # (libamdhip64.so.7).  Loaded first, it is the one libsbag binds to; loaded
            # after libsbag, torch would bring a second HIP/HSA runtime into the process
            # and device pointers of one (torch tensors handed to the multi-GPU
            # aggregation) would be foreign to the other.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
        sig = {
            "sbag_device_count": [P],
            "sbag_ctx_create": [i32, P],
            "sbag_ctx_destroy": [P],
            "sbag_sample": [P, ctypes.POINTER(SamplerParams), P, i32, i64, P],
            "sbag_subspace": [dbl, i32, i64, P, P],
            "sbag_dataset_create": [P, i64, i32, P, P, P],
            "sbag_dataset_synthetic": [P, i64, i32, ctypes.c_uint64, i32, P],
            "sbag_dataset_create_csr": [P, i64, i32, P, P, P, P, P],
            "sbag_dataset_create_columns": [P, i64, i32, i32, P, P, P],
            "sbag_dataset_info": [P, P, P],
            "sbag_dataset_labels": [P, P],
            "sbag_dataset_features": [P, i64, i64, P],
            "sbag_dataset_free": [P],
            "sbag_dataset_set_labels": [P, P],
            "sbag_dataset_layout": [P, P, P, P, P, P],
            "sbag_dataset_export": [P, P, i32, P, P, P],
            "sbag_dataset_import": [P, i64, i32, i32, i32, P, i32, P, P, P, P],
            "sbag_fit": [P, P, ctypes.POINTER(FitParams), P],
            "sbag_fit_booster": [P, P, P, ctypes.POINTER(BoosterParams), P],
            "sbag_sample_boosted": [P, P, i64, P, i32, i64, P],
            "sbag_sample_boosted_stats": [P, ctypes.POINTER(BoostedStats)],
            "sbag_fit_bag": [P, P, ctypes.POINTER(BoosterParams), P],
            "sbag_dataset_create_stacked": [P, P, P, P],
            "sbag_predict_stacked": [P, P, P, P, i64, i32, P],
            "sbag_predict_stacked_dataset": [P, P, P, P, P],
            "sbag_forest_num_trees": [P, P],
            "sbag_forest_tree_info": [P, i32, P, P, P, P],
            "sbag_forest_subspace": [P, i32, P],
            "sbag_forest_nodes": [P, i32, P, P],
            "sbag_forest_create": [i32, P, P, P, P, i32, P],
            "sbag_forest_free": [P],
            "sbag_forest_num_classes": [P, P],
            "sbag_forest_create_stats": [i32, P, P, P, P, i32, P, P, P],
            "sbag_predict_raw": [P, P, P, i64, i32, i32, i32, P],
            "sbag_predict_raw_dataset": [P, P, P, i32, i32, P],
            "sbag_predict_oob_raw": [P, P, P, ctypes.POINTER(SamplerParams), P, i32, i32, i32, P, P],
            "sbag_predict_weighted": [P, P, P, i64, i32, i32, P, i32, i32, P],
            "sbag_predict_weighted_dataset": [P, P, P, i32, P, i32, i32, P],
            "sbag_forest_timing": [P, ctypes.POINTER(Timing)],
            "sbag_predict": [P, P, P, i64, i32, i32, P, P],
            "sbag_predict_dataset": [P, P, P, i32, P],
            "sbag_aggregate": [P, P, i32, i64, i32, P],
            "sbag_predict_dataset_device": [P, P, P, i32, i32, P],
            "sbag_aggregate_device": [P, P, i32, i32, i64, i32, i32, i32, P],
            "sbag_predict_oob": [P, P, P, ctypes.POINTER(SamplerParams), P, i32, i32, P, P],
            "sbag_eval_staged": [P, P, P, ctypes.POINTER(SamplerParams), P, i32, i32, P],
            "sbag_predict_oob_permuted": [P, P, P, ctypes.POINTER(SamplerParams), P, i32, i32, P, i32, P, P,
                                          P, P],
        }
        for name, args in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        L.sbag_last_error.restype = ctypes.c_char_p
        L.sbag_last_error.argtypes = []
        L.sbag_version.restype = ctypes.c_char_p
        L.sbag_version.argtypes = []
        _lib = L
    return _lib


def check(rc):
    if rc == SBAG_OK:
        return
    msg = lib().sbag_last_error().decode(errors="replace")
    if rc == SBAG_EINVAL:
        raise IllegalArgumentException(rc, msg)
    raise SparkException(rc, msg)


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Context:
    """One device context (sbag_ctx).  The library serializes calls on a context (sbag.h)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        check(lib().sbag_ctx_create(device, ctypes.byref(self._h)))
        self.device = device
        self._datasets = weakref.WeakSet()  # freed before the context (sbag.h ownership)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            for ds in list(self._datasets):
                ds.free()
            lib().sbag_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def device_count():
    n = ctypes.c_int32()
    check(lib().sbag_device_count(ctypes.byref(n)))
    return n.value


class DeviceDataset:
    """Label + features columns resident in HBM (sbag_dataset)."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle
        ctx._datasets.add(self)

    @classmethod
    def from_numpy(cls, X, y, ctx=None):
        ctx = ctx or default_context()
        X = np.ascontiguousarray(X, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        h = ctypes.c_void_p()
        check(lib().sbag_dataset_create(ctx.handle, X.shape[0], X.shape[1], ptr(X), ptr(y),
                                        ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_csr(cls, rows, y, ctx=None):
        """SparseVector rows (libsvm.SparseRows or a scipy.sparse CSR matrix): absent
        entries are 0.0; no dense copy is made (sbag_dataset_create_csr)."""
        ctx = ctx or default_context()
        n, f = rows.shape
        indptr = np.ascontiguousarray(rows.indptr, np.int64)
        indices = np.ascontiguousarray(rows.indices, np.int32)
        values = np.ascontiguousarray(rows.data, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        if len(indptr) != n + 1 or len(y) != n:
            raise IllegalArgumentException(SBAG_EINVAL, "indptr / labels do not match the row count")
        h = ctypes.c_void_p()
        check(lib().sbag_dataset_create_csr(ctx.handle, n, f, ptr(indptr), ptr(indices), ptr(values),
                                            ptr(y), ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_columns(cls, columns, y, ctx=None):
        """Columnar features: a list of F arrays of N values (fp64, fp32 or u8, one dtype),
        e.g. Arrow / Parquet column chunks (sbag_dataset_create_columns)."""
        ctx = ctx or default_context()
        kinds = {np.dtype(np.float64): COL_F64, np.dtype(np.float32): COL_F32,
                 np.dtype(np.uint8): COL_U8}
        cols = [np.ascontiguousarray(c) for c in columns]
        dts = {c.dtype for c in cols}
        if len(dts) != 1 or next(iter(dts)) not in kinds:
            raise IllegalArgumentException(SBAG_EINVAL, "columns must share one of fp64 / fp32 / u8")
        y = np.ascontiguousarray(y, np.float64)
        if any(len(c) != len(y) for c in cols):
            raise IllegalArgumentException(SBAG_EINVAL, "columns and labels differ in length")
        arr = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        h = ctypes.c_void_p()
        check(lib().sbag_dataset_create_columns(ctx.handle, len(y), len(cols), kinds[cols[0].dtype],
                                                arr, ptr(y), ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def synthetic(cls, num_rows, num_features, seed=20261015, num_classes=0, ctx=None):
        ctx = ctx or default_context()
        h = ctypes.c_void_p()
        check(lib().sbag_dataset_synthetic(ctx.handle, num_rows, num_features, seed, num_classes,
                                           ctypes.byref(h)))
        return cls(ctx, h)

    @property
    def handle(self):
        return self._h

    @property
    def shape(self):
        n, f = ctypes.c_int64(), ctypes.c_int32()
        check(lib().sbag_dataset_info(self._h, ctypes.byref(n), ctypes.byref(f)))
        return n.value, f.value

    def labels(self):
        y = np.zeros(self.shape[0], np.float64)
        check(lib().sbag_dataset_labels(self._h, ptr(y)))
        return y

    def set_labels(self, y):
        """Replace the label column (sbag_dataset_set_labels); non-dyadic regression labels
        are then fitted with Spark's row-order fp64 sums."""
        y = np.ascontiguousarray(y, np.float64)
        if y.shape != (self.shape[0],):
            raise IllegalArgumentException(SBAG_EINVAL, "labels do not match the row count")
        check(lib().sbag_dataset_set_labels(self._h, ptr(y)))

    def layout(self):
        """(num_rows, num_features, row_stride, code_bytes, dict_values) of the codes."""
        n, f, s, cb, dv = (ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(),
                           ctypes.c_int64())
        check(lib().sbag_dataset_layout(self._h, ctypes.byref(n), ctypes.byref(f), ctypes.byref(s),
                                        ctypes.byref(cb), ctypes.byref(dv)))
        return n.value, f.value, s.value, cb.value, dv.value

    def codes_nbytes(self):
        n, _, s, cb, _ = self.layout()
        return n * s * cb

    def export(self, codes_ptr=None, codes_on_device=False):
        """Export for replication: the codes into `codes_ptr` (device memory of this
        dataset's device when codes_on_device, else host memory of codes_nbytes() bytes;
        None: skipped), and (dict, dict_off, labels) as numpy arrays."""
        n, f, _, _, dv = self.layout()
        d = np.zeros(max(dv, 1), np.float64)
        off = np.zeros(f + 1, np.int64)
        y = np.zeros(n, np.float64)
        check(lib().sbag_dataset_export(self._h, ctypes.c_void_p(codes_ptr) if codes_ptr else None,
                                        1 if codes_on_device else 0, ptr(d), ptr(off), ptr(y)))
        return d[:dv], off, y

    @classmethod
    def import_codes(cls, ctx, layout, codes_ptr, codes_on_device, dict_values, dict_off, y):
        """A dataset from exported pieces (sbag_dataset_import): `layout` as layout()
        returns it, the codes at codes_ptr (device memory of ctx's device or host)."""
        n, f, s, cb, _ = layout
        d = np.ascontiguousarray(dict_values, np.float64)
        off = np.ascontiguousarray(dict_off, np.int64)
        y = np.ascontiguousarray(y, np.float64)
        h = ctypes.c_void_p()
        check(lib().sbag_dataset_import(ctx.handle, n, f, s, cb, ctypes.c_void_p(codes_ptr),
                                        1 if codes_on_device else 0, ptr(d), ptr(off), ptr(y),
                                        ctypes.byref(h)))
        return cls(ctx, h)

    def stacked(self, forest, ctx=None):
        """The level-1 dataset of a stacking fit (sbag_dataset_create_stacked): feature k of
        row r is tree k of `forest`'s prediction of row r, the labels are this dataset's.
        Built on the device; equal to from_numpy of the per-tree prediction matrix."""
        ctx = ctx or self.ctx
        h = ctypes.c_void_p()
        check(lib().sbag_dataset_create_stacked(ctx.handle, self._h, forest.handle, ctypes.byref(h)))
        return DeviceDataset(ctx, h)

    def features(self, row_begin=0, row_end=None):
        n, f = self.shape
        row_end = n if row_end is None else row_end
        X = np.zeros((row_end - row_begin, f), np.float64)
        check(lib().sbag_dataset_features(self._h, row_begin, row_end, ptr(X)))
        return X

    def free(self):
        if self._h:
            lib().sbag_dataset_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class NativeForest:
    """Fitted trees (sbag_forest): pre-order NodeData arrays + subspaces."""

    def __init__(self, handle, impurity):
        self._h, self.impurity = handle, impurity

    @property
    def handle(self):
        return self._h

    def __len__(self):
        n = ctypes.c_int32()
        check(lib().sbag_forest_num_trees(self._h, ctypes.byref(n)))
        return n.value

    def tree(self, t):
        nn, ns, sl, ex = (ctypes.c_int32() for _ in range(4))
        check(lib().sbag_forest_tree_info(self._h, t, ctypes.byref(nn), ctypes.byref(ns),
                                          ctypes.byref(sl), ctypes.byref(ex)))
        nodes = np.zeros(nn.value, NODE_DTYPE)
        stats = np.zeros((nn.value, max(ns.value, 1)), np.float64)
        check(lib().sbag_forest_nodes(self._h, t, ptr(nodes), ptr(stats)))
        return nodes, stats[:, : ns.value]

    def subspace(self, t):
        nn, ns, sl, ex = (ctypes.c_int32() for _ in range(4))
        check(lib().sbag_forest_tree_info(self._h, t, ctypes.byref(nn), ctypes.byref(ns),
                                          ctypes.byref(sl), ctypes.byref(ex)))
        idx = np.zeros(max(sl.value, 1), np.int32)
        check(lib().sbag_forest_subspace(self._h, t, ptr(idx)))
        return idx[: sl.value]

    def exact(self, t):
        nn, ns, sl, ex = (ctypes.c_int32() for _ in range(4))
        check(lib().sbag_forest_tree_info(self._h, t, ctypes.byref(nn), ctypes.byref(ns),
                                          ctypes.byref(sl), ctypes.byref(ex)))
        return bool(ex.value)

    def timing(self):
        t = Timing()
        check(lib().sbag_forest_timing(self._h, ctypes.byref(t)))
        return t.as_dict()

    @property
    def num_classes(self):
        """Class count of a gini forest (the columns predict_raw fills); 0 for variance."""
        n = ctypes.c_int32()
        check(lib().sbag_forest_num_classes(self._h, ctypes.byref(n)))
        return n.value

    @classmethod
    def from_trees(cls, trees, subspaces, impurity, stats=None):
        """A forest from node arrays; with `stats` (one [num_nodes, num_stats] array per
        tree, the impurityStats column) through sbag_forest_create_stats, which keeps them
        (RAW_LEAF needs a gini forest's class counts)."""
        nn = np.array([len(n) for n in trees], np.int32)
        nodes = np.ascontiguousarray(np.concatenate(trees).astype(NODE_DTYPE))
        sl = np.array([len(s) for s in subspaces], np.int32)
        subs = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in subspaces]))
        h = ctypes.c_void_p()
        if stats is None:
            check(lib().sbag_forest_create(len(trees), ptr(nn), ptr(nodes), ptr(sl), ptr(subs),
                                           impurity, ctypes.byref(h)))
            return cls(h, impurity)
        st = [np.asarray(s, np.float64).reshape(len(n), -1) for s, n in zip(stats, trees)]
        if len(st) != len(trees):
            raise IllegalArgumentException(SBAG_EINVAL, "one stats array per tree")
        ns = np.array([s.shape[1] for s in st], np.int32)
        flat = np.ascontiguousarray(np.concatenate([s.reshape(-1) for s in st] + [np.zeros(1)]))
        check(lib().sbag_forest_create_stats(len(trees), ptr(nn), ptr(nodes), ptr(sl), ptr(subs),
                                             impurity, ptr(ns), ptr(flat), ctypes.byref(h)))
        return cls(h, impurity)

    def free(self):
        if self._h:
            lib().sbag_forest_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sample(ctx, replacement, ratio, seed, learner_begin, learner_end, num_rows,
           partition_offsets=None):
    p = SamplerParams(int(replacement), 0, float(ratio), int(seed), learner_begin, learner_end)
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    out = np.zeros((learner_end - learner_begin, num_rows), np.uint8)
    check(lib().sbag_sample(ctx.handle, ctypes.byref(p), ptr(off), P, num_rows, ptr(out)))
    return out


def subspace(ratio, num_features, seed):
    idx = np.zeros(max(num_features, 1), np.int32)
    n = ctypes.c_int32()
    check(lib().sbag_subspace(float(ratio), num_features, int(seed), ptr(idx), ctypes.byref(n)))
    return idx[: n.value].copy()


def fit(ctx, dataset, *, replacement, sample_ratio, seed, learner_begin, learner_end,
        subspace_ratio=1.0, subspace_bug_compat=True, partition_offsets=None, max_depth=5,
        max_bins=32, min_instances_per_node=1, min_info_gain=0.0, impurity=IMPURITY_VARIANCE,
        tree_seed=None):
    if tree_seed is None:
        tree_seed = DT_SEED_CLASSIFIER if impurity == IMPURITY_GINI else DT_SEED_REGRESSOR
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    fp = FitParams(SamplerParams(int(replacement), 0, float(sample_ratio), int(seed),
                                 learner_begin, learner_end),
                   float(subspace_ratio), int(subspace_bug_compat), P,
                   off.ctypes.data if off is not None else None,
                   TreeParams(max_depth, max_bins, min_instances_per_node, impurity,
                              float(min_info_gain), int(tree_seed)))
    h = ctypes.c_void_p()
    check(lib().sbag_fit(ctx.handle, dataset.handle, ctypes.byref(fp), ctypes.byref(h)))
    return NativeForest(h, impurity)


def fit_booster(ctx, dataset, labels, counts, subspace, *, partition_offsets=None, max_depth=5,
                max_bins=32, min_instances_per_node=1, min_info_gain=0.0, tree_seed=None):
    """One GBM base-learner fit (sbag_fit_booster): DecisionTreeRegressor on the subbag
    `counts` (u8 per row) sliced to `subspace`, with fp64 labels (pseudo-residuals)."""
    if tree_seed is None:
        tree_seed = DT_SEED_REGRESSOR
    labels = np.ascontiguousarray(labels, np.float64)
    counts = np.ascontiguousarray(counts, np.uint8)
    sub = np.ascontiguousarray(subspace, np.int32)
    n = dataset.shape[0]
    if len(labels) != n or len(counts) != n:
        raise IllegalArgumentException(SBAG_EINVAL, "labels / counts do not match the row count")
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    bp = BoosterParams(counts.ctypes.data, sub.ctypes.data, len(sub), P,
                       off.ctypes.data if off is not None else None,
                       TreeParams(max_depth, max_bins, min_instances_per_node, IMPURITY_VARIANCE,
                                  float(min_info_gain), int(tree_seed)))
    h = ctypes.c_void_p()
    check(lib().sbag_fit_booster(ctx.handle, dataset.handle, ptr(labels), ctypes.byref(bp),
                                 ctypes.byref(h)))
    return NativeForest(h, IMPURITY_VARIANCE)


def sample_boosted(ctx, mean, seed, partition_offsets=None):
    """The boosted bag (sbag_sample_boosted): row j of partition i draws one
    Poisson(mean[r]) from a Well19937c seeded with seed + i + j; rows with mean 0.0 get 0."""
    mean = np.ascontiguousarray(mean, np.float64).reshape(-1)
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    seed = ((int(seed) + 2**63) % 2**64) - 2**63  # Long arithmetic wraps
    out = np.zeros(len(mean), np.uint8)
    check(lib().sbag_sample_boosted(ctx.handle, ptr(mean), seed, ptr(off), P, len(mean), ptr(out)))
    return out


def sample_boosted_stats(ctx):
    """Rows per path and kernel times of the context's last sample_boosted."""
    s = BoostedStats()
    check(lib().sbag_sample_boosted_stats(ctx.handle, ctypes.byref(s)))
    return s.as_dict()


def fit_bag(ctx, dataset, counts, subspace, *, impurity, partition_offsets=None, max_depth=5,
            max_bins=32, min_instances_per_node=1, min_info_gain=0.0, tree_seed=None):
    """One tree on the bag `counts` (u8 per row) sliced to `subspace`, with the dataset's own
    labels (sbag_fit_bag): the Boosting estimators' base-learner fit."""
    if tree_seed is None:
        tree_seed = DT_SEED_CLASSIFIER if impurity == IMPURITY_GINI else DT_SEED_REGRESSOR
    counts = np.ascontiguousarray(counts, np.uint8)
    sub = np.ascontiguousarray(subspace, np.int32)
    if len(counts) != dataset.shape[0]:
        raise IllegalArgumentException(SBAG_EINVAL, "counts do not match the row count")
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    bp = BoosterParams(counts.ctypes.data, sub.ctypes.data, len(sub), P,
                       off.ctypes.data if off is not None else None,
                       TreeParams(max_depth, max_bins, min_instances_per_node, impurity,
                                  float(min_info_gain), int(tree_seed)))
    h = ctypes.c_void_p()
    check(lib().sbag_fit_bag(ctx.handle, dataset.handle, ctypes.byref(bp), ctypes.byref(h)))
    return NativeForest(h, impurity)


def predict(ctx, forest, X, agg, per_tree=False):
    X = np.ascontiguousarray(X, np.float64)
    out = np.zeros(X.shape[0], np.float64)
    pt = np.zeros((len(forest), X.shape[0]), np.float64) if per_tree else None
    check(lib().sbag_predict(ctx.handle, forest.handle, ptr(X), X.shape[0], X.shape[1], agg,
                             ptr(out), ptr(pt)))
    return (out, pt) if per_tree else out


def predict_dataset(ctx, forest, dataset, agg):
    out = np.zeros(dataset.shape[0], np.float64)
    check(lib().sbag_predict_dataset(ctx.handle, forest.handle, dataset.handle, agg, ptr(out)))
    return out


def predict_oob(ctx, forest, dataset, *, replacement, sample_ratio, seed, learner_begin, learner_end,
                partition_offsets=None, agg):
    """Out-of-bag predictions (sbag_predict_oob) of `forest` on the dataset it was fitted
    on, the sampler arguments and partition offsets being the fit's: (pred fp64 [N], NaN
    where no learner left the row out; n_oob int32 [N])."""
    p = SamplerParams(int(replacement), 0, float(sample_ratio), int(seed), learner_begin, learner_end)
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    n = dataset.shape[0]
    out = np.zeros(n, np.float64)
    n_oob = np.zeros(n, np.int32)
    check(lib().sbag_predict_oob(ctx.handle, forest.handle, dataset.handle, ctypes.byref(p), ptr(off),
                                 P, agg, ptr(out), ptr(n_oob)))
    return out, n_oob


def eval_staged(ctx, forest, dataset, *, agg, replacement=None, sample_ratio=None, seed=None,
                learner_begin=None, learner_end=None, partition_offsets=None):
    """Staged evaluation (sbag_eval_staged): a structured array [trees] (STAGE_DTYPE: covered,
    correct, sum_se, sum_ae), record l the score of the forest's first l + 1 trees against the
    dataset's labels.  With the fit's sampler arguments (predict_oob's) every stage is the
    out-of-bag one; with all of them None no learner is masked (the held-out curve) and
    partition_offsets is ignored."""
    sampler = (replacement, sample_ratio, seed, learner_begin, learner_end)
    p = None
    if any(a is not None for a in sampler):
        if any(a is None for a in sampler):
            raise IllegalArgumentException(SBAG_EINVAL, "give every sampler argument or none")
        p = SamplerParams(int(replacement), 0, float(sample_ratio), int(seed), learner_begin, learner_end)
    off = None
    P = 1
    if p is not None and partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    out = np.zeros(len(forest), STAGE_DTYPE)
    check(lib().sbag_eval_staged(ctx.handle, forest.handle, dataset.handle,
                                 ctypes.byref(p) if p is not None else None, ptr(off), P, agg, ptr(out)))
    return out


def predict_oob_permuted(ctx, forest, dataset, *, replacement, sample_ratio, seed, learner_begin, learner_end,
                         partition_offsets=None, agg, features, src_rows):
    """Out-of-bag predictions under permuted features (sbag_predict_oob_permuted): slot k is
    predict_oob with feature features[k] of row r read from row src_rows[k][r] (int32
    [K, N], any map into [0, N)).  Returns (perm_pred fp64 [K, N], base_pred fp64 [N],
    n_oob int32 [N]); base_pred and n_oob are predict_oob's."""
    p = SamplerParams(int(replacement), 0, float(sample_ratio), int(seed), learner_begin, learner_end)
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    n = dataset.shape[0]
    feats = np.ascontiguousarray(features, np.int32).reshape(-1)
    K = len(feats)
    src = np.ascontiguousarray(src_rows, np.int32).reshape(K, n)
    out = np.zeros((K, n), np.float64)
    base = np.zeros(n, np.float64)
    n_oob = np.zeros(n, np.int32)
    check(lib().sbag_predict_oob_permuted(ctx.handle, forest.handle, dataset.handle, ctypes.byref(p), ptr(off),
                                          P, agg, ptr(feats), K, ptr(src), ptr(out), ptr(base), ptr(n_oob)))
    return out, base, n_oob


def _raw_width(forest, num_classes):
    return forest.num_classes if num_classes is None else int(num_classes)


def predict_raw(ctx, forest, X, kind, num_classes=None):
    """Per-class raw predictions of host rows (sbag_predict_raw): fp64 [N, num_classes]
    (default: the forest's class count); RAW_VOTES counts the trees per class, RAW_LEAF sums
    their leaf class fractions in learner order."""
    X = np.ascontiguousarray(X, np.float64)
    C = _raw_width(forest, num_classes)
    raw = np.zeros((X.shape[0], max(C, 0)), np.float64)
    check(lib().sbag_predict_raw(ctx.handle, forest.handle, ptr(X), X.shape[0], X.shape[1], kind, C,
                                 ptr(raw)))
    return raw


def predict_raw_dataset(ctx, forest, dataset, kind, num_classes=None):
    """predict_raw over a device dataset (sbag_predict_raw_dataset)."""
    C = _raw_width(forest, num_classes)
    raw = np.zeros((dataset.shape[0], max(C, 0)), np.float64)
    check(lib().sbag_predict_raw_dataset(ctx.handle, forest.handle, dataset.handle, kind, C, ptr(raw)))
    return raw


def predict_oob_raw(ctx, forest, dataset, *, replacement, sample_ratio, seed, learner_begin, learner_end,
                    partition_offsets=None, kind, num_classes=None):
    """Out-of-bag raw predictions (sbag_predict_oob_raw), the sampler arguments as
    predict_oob's: (raw fp64 [N, num_classes] over the learners that left the row out, a row
    of 0.0 where there is none; n_oob int32 [N], predict_oob's)."""
    p = SamplerParams(int(replacement), 0, float(sample_ratio), int(seed), learner_begin, learner_end)
    off = None
    P = 1
    if partition_offsets is not None:
        off = np.ascontiguousarray(partition_offsets, np.int64)
        P = len(off) - 1
    n = dataset.shape[0]
    C = _raw_width(forest, num_classes)
    raw = np.zeros((n, max(C, 0)), np.float64)
    n_oob = np.zeros(n, np.int32)
    check(lib().sbag_predict_oob_raw(ctx.handle, forest.handle, dataset.handle, ctypes.byref(p), ptr(off),
                                     P, kind, C, ptr(raw), ptr(n_oob)))
    return raw, n_oob


def predict_weighted(ctx, forest, X, kind, weights, num_cols=1):
    """Weighted sums over the trees of host rows (sbag_predict_weighted): fp64 [N, num_cols].
    W_DOT: out[r, t % num_cols] += tree_t(r) * weights[t] in forest order, the product rounded
    first; W_CLASS: out[r, class tree_t(r) predicts] += weights[t]."""
    X = np.ascontiguousarray(X, np.float64)
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    out = np.zeros((X.shape[0], max(int(num_cols), 0)), np.float64)
    check(lib().sbag_predict_weighted(ctx.handle, forest.handle, ptr(X), X.shape[0], X.shape[1], kind,
                                      ptr(w), len(w), int(num_cols), ptr(out)))
    return out


def predict_weighted_dataset(ctx, forest, dataset, kind, weights, num_cols=1):
    """predict_weighted over a device dataset (sbag_predict_weighted_dataset): no feature
    leaves the device."""
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    out = np.zeros((dataset.shape[0], max(int(num_cols), 0)), np.float64)
    check(lib().sbag_predict_weighted_dataset(ctx.handle, forest.handle, dataset.handle, kind, ptr(w),
                                              len(w), int(num_cols), ptr(out)))
    return out


def predict_stacked(ctx, base, stack, X_or_dataset):
    """StackingModel.predict: the one tree of `stack` over the predictions of `base`'s trees
    (sbag_predict_stacked for host rows, sbag_predict_stacked_dataset for a DeviceDataset)."""
    if isinstance(X_or_dataset, DeviceDataset):
        ds = X_or_dataset
        out = np.zeros(ds.shape[0], np.float64)
        check(lib().sbag_predict_stacked_dataset(ctx.handle, base.handle, stack.handle, ds.handle,
                                                 ptr(out)))
        return out
    X = np.ascontiguousarray(X_or_dataset, np.float64)
    out = np.zeros(X.shape[0], np.float64)
    check(lib().sbag_predict_stacked(ctx.handle, base.handle, stack.handle, ptr(X), X.shape[0],
                                     X.shape[1], ptr(out)))
    return out


def aggregate(ctx, votes, agg):
    votes = np.ascontiguousarray(votes, np.float64)
    out = np.zeros(votes.shape[1], np.float64)
    check(lib().sbag_aggregate(ctx.handle, ptr(votes), votes.shape[0], votes.shape[1], agg,
                               ptr(out)))
    return out


def predict_dataset_device(ctx, forest, dataset, out_kind, vote_bytes, d_out):
    """Device outputs for the multi-GPU aggregation (distributed.transform): d_out is a
    device pointer on the context's device (OUT_SUM: fp64 [N]; OUT_VOTES: [trees x N]
    u8 / u16 class ids)."""
    check(lib().sbag_predict_dataset_device(ctx.handle, forest.handle, dataset.handle, out_kind,
                                            vote_bytes, ctypes.c_void_p(d_out)))


def aggregate_device(ctx, d_in, in_bytes, K, N, agg, num_learners, num_classes, d_out):
    """Ordered mean of K fp64 partial-sum rows / num_learners, or breeze mode of K u8 /
    u16 vote rows; device pointers in and out (fp64 [N])."""
    check(lib().sbag_aggregate_device(ctx.handle, ctypes.c_void_p(d_in), in_bytes, K, N, agg,
                                      num_learners, num_classes, ctypes.c_void_p(d_out)))
