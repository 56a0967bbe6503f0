"""BoostingClassifier (SAMME) / BoostingRegressor (AdaBoost.R2) and their models: the
reference's Boosting family on a DecisionTree base learner, with the boosted bag, the base
learner fit and the tree walks on the device.

Mirror of (paths relative to the reference's core/src/main/scala/org/apache/spark/):

  BoostingClassifier.train       ml/classification/BoostingClassifier.scala:173-378
  BoostingClassificationModel    ml/classification/BoostingClassifier.scala:414-447
  BoostingRegressor.train        ml/regression/BoostingRegressor.scala:135-336
  BoostingRegressionModel        ml/regression/BoostingRegressor.scala:373-411
  loss functions                 BoostingClassifier.scala:72-77, BoostingRegressor.scala:73-82
  params, probabilize, avgLoss, beta, weight, updateWeights, extractBoostedBag,
  evaluateOnValidation, terminate / terminateVal      ml/boosting/BoostingParams.scala:34-199
  persistence                    BoostingClassifier.scala:455-504, BoostingRegressor.scala:421-470

Per boosting iteration (one step of the reference's trainBoosters recursion):
  * probabilize: proba = weight / sum(weight), the SQL sum being each partition's
    left-to-right fp64 sum merged in partition order; poisson mean = proba * numLines;
  * the bag: sbag_sample_boosted -- row j of partition i draws Poisson(mean) from a
    Well19937c reseeded with seed + i + j (k_boost_fast / k_boost_ring);
  * the booster: sbag_fit_bag -- DecisionTreeClassifier (gini) or DecisionTreeRegressor on
    the replicated rows, the labels already resident with the dataset;
  * its predictions on the resident training rows (sbag_predict_dataset) -> loss:
      classifier  1 - exp(-(0 | 1)), 1 where label != prediction;
      regressor   coalesce(loss(|label - prediction| / maxError), 0.0): SQL division by a
                  zero maxError is NULL, so every loss is then 0;
  * avgLoss = sum(loss * proba), beta = avgl / ((1 - avgl) * (numClasses - 1)) (numClasses
    2 for the regressor), weight = log(1 / beta), or 1.0 when beta == 0;
  * updateWeights: weight * pow(beta, 1 - loss);
  * evaluateOnValidation: both estimators evaluate a BoostingRegressionModel (the weighted
    mean of the boosters' predictions); the classifier compares that mean with the label by
    `===` (its overload never builds a classification model): reproduced as it runs;
  * terminate (numClasses as a Double), the next iteration's seed is seed + iter, and the
    last numTry boosters are dropped at the end.

JVM math.  `exp`, `pow` and `log` on the host are numpy's (the platform libm); the JVM
evaluates breeze.numerics.exp / math.log through StrictMath (fdlibm) and SQL `pow` through
StrictMath.pow.  They agree to the last bit for almost every argument but are not
guaranteed to; the same caveat gbm.py carries for its sqrt / exp / log.  Everything on the
device -- the bag given the means, the tree given the bag, the walks -- is bit-exact given
the same inputs, which is what the tests pin.
"""
import os
import warnings

import numpy as np

from . import _native as nat
from . import persistence as sp
from .libsvm import is_sparse
from .ml import (DecisionTreeClassifier, DecisionTreeModel, DecisionTreeRegressor, Frame, Params,
                 _DecisionTreeEstimator, java_string_hash)

CLASSIFIER_LOSSES = ("exponential",)
REGRESSOR_LOSSES = ("exponential", "squared", "absolute")
DOUBLE_MAX = np.finfo(np.float64).max


def loss_function(loss):
    """Boosting{Classifier,Regressor}Params.lossFunction, elementwise fp64."""
    if loss == "exponential":
        return lambda e: 1.0 - np.exp(-e)
    if loss == "absolute":
        return lambda e: e
    if loss == "squared":
        return lambda e: np.power(e, 2)
    raise RuntimeError(f"Boosting was given bad loss type: {loss}")


def partition_sum(x, part):
    """SQL sum() of a column: every partition's left-to-right fp64 sum, the partial sums
    merged in partition order (an empty partition has no partial sum)."""
    x = np.asarray(x, np.float64)
    total = None
    for p in range(len(part) - 1):
        seg = x[part[p]:part[p + 1]]
        if len(seg):
            s = float(np.cumsum(seg)[-1])
            total = s if total is None else total + s
    return 0.0 if total is None else total


def beta(avgl, num_classes=2):
    """BoostingParams.beta."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(avgl) / ((np.float64(1) - avgl) * np.float64(num_classes - 1)))


def weight(b):
    """BoostingParams.weight."""
    if b == 0.0:
        return 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.log(np.float64(1) / np.float64(b)))


def terminate_val(with_validation, error, verror, tol, num_round, num_try, it):
    """BoostingParams.terminateVal -> (iter, error, numTry)."""
    if with_validation:
        if verror < error * (1 - tol):
            return it - 1, verror, 0
        if num_try == num_round - 1:
            return 0, 0.0, num_try + 1
        return it - 1, error, num_try + 1
    return it - 1, 0.0, 0


def terminate(avgl, with_validation, error, verror, tol, num_round, num_try, it, num_classes=2.0):
    """BoostingParams.terminate -> (iter, error, numTry)."""
    if avgl > (num_classes - 1.0) / num_classes:
        return 0, 0.0, 1
    if avgl == 0.0:
        return 0, 0.0, 0
    return terminate_val(with_validation, error, verror, tol, num_round, num_try, it)


def _rows_and_ctx(dataset, device):
    if isinstance(dataset, nat.DeviceDataset):
        return dataset.features(), dataset.ctx
    X = dataset.features if isinstance(dataset, Frame) else dataset
    if is_sparse(X):
        X = X.toarray() if hasattr(X, "toarray") else X.to_dense()
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[None, :]
    return X, nat.default_context(device)


class _BoostingParams(Params):
    _defaults = {"numBaseLearners": 10, "tol": 1e-3, "numRound": 5, "loss": "exponential",
                 "validationIndicatorCol": None, "weightCol": None, "baseLearner": None,
                 "labelCol": "label", "featuresCol": "features", "predictionCol": "prediction",
                 "seed": None}
    _validators = {"numBaseLearners": lambda x: int(x) >= 1, "tol": lambda x: float(x) >= 0.0,
                   "numRound": lambda x: int(x) >= 1}
    _classification = False

    def getLoss(self):
        return str(self.get("loss")).lower()

    def getNumBaseLearners(self):
        return self.get("numBaseLearners")

    def getTol(self):
        return self.get("tol")

    def getNumRound(self):
        return self.get("numRound")

    def getSeed(self):
        return self.get("seed")

    def getBaseLearner(self):
        return self.get("baseLearner")

    def _base_learner(self):
        return self.get("baseLearner") or (DecisionTreeClassifier() if self._classification
                                           else DecisionTreeRegressor())

    def _check_new_path(self, path):
        if os.path.exists(path):
            raise nat.IllegalArgumentException(
                nat.SBAG_EINVAL, f"Path {path} already exists. To overwrite it, please use "
                                 "write.overwrite().save(path) for Scala and use "
                                 "write().overwrite().save(path) for Java and Python.")

    def _save_params(self, path, extra=None):
        """Boosting*Params.saveImpl: metadata without baseLearner, then learner/."""
        params = {k: v for k, v in self.extractParamMap().items()
                  if k != "baseLearner" and v is not None}
        defaults = {k: v for k, v in self._defaults.items() if v is not None and k != "baseLearner"}
        sp.save_metadata(path, self._spark_class, self.uid, params, defaults, extra)
        self._base_learner().save(os.path.join(path, "learner"))


class _BoostingModel(_BoostingParams):
    """weights and models of Boosting*Model, and their shared reader / writer."""

    def __init__(self, weights, models, uid=None, num_features=None):
        super().__init__(uid)
        self.weights = [float(w) for w in weights]
        self.models = list(models)
        self._num_features = int(num_features or 0)  # of the rows the boosters were fitted on
        self._forest = None

    @property
    def numBaseModels(self):
        return len(self.models)

    def _subspace(self, m):
        # the boosters see every feature (the reference slices nothing here)
        nf = int(m.nodes["feature"].max()) + 1 if len(m.nodes) else 0
        return np.arange(max(nf, self._num_features, 1), dtype=np.int32)

    def native_forest(self):
        if self._forest is None:
            imp = nat.IMPURITY_GINI if self._classification else nat.IMPURITY_VARIANCE
            self._forest = nat.NativeForest.from_trees([m.nodes for m in self.models],
                                                       [self._subspace(m) for m in self.models], imp)
        return self._forest

    def per_tree(self, dataset, device=0):
        """Every booster's prediction of every row, from one sbag_predict call:
        (fp64 [numBaseModels, N], N)."""
        X, ctx = _rows_and_ctx(dataset, device)
        if not self.models:
            return np.zeros((0, X.shape[0])), X.shape[0]
        agg = nat.AGG_MODE if self._classification else nat.AGG_MEAN
        _, pt = nat.predict(ctx, self.native_forest(), X, agg, per_tree=True)
        return pt, X.shape[0]

    def _weighted(self, dataset, device, kind, num_cols):
        """sbag_predict_weighted(_dataset) over the boosters and their weights, fp64
        [N, num_cols]; a DeviceDataset stays resident.  (None, N) for a model without boosters."""
        if isinstance(dataset, nat.DeviceDataset):
            if not self.models:
                return None, dataset.shape[0]
            return nat.predict_weighted_dataset(dataset.ctx, self.native_forest(), dataset, kind,
                                                self.weights, num_cols), dataset.shape[0]
        X, ctx = _rows_and_ctx(dataset, device)
        if not self.models:
            return None, X.shape[0]
        return nat.predict_weighted(ctx, self.native_forest(), X, kind, self.weights, num_cols), X.shape[0]

    def predict(self, features):
        return float(self.transform(np.asarray(features, np.float64)[None, :])[0])

    def _extra_metadata(self):
        return {"numBaseModels": self.numBaseModels}

    def save(self, path):
        """Boosting*ModelWriter.saveImpl: metadata (+ numBaseModels, the classifier's
        numClasses), learner/, model-$idx (the tree), data-$idx ({weight})."""
        self._check_new_path(path)
        self._save_params(path, self._extra_metadata())
        bl = self._base_learner()
        tree_params = dict(bl._other_params, **bl._values)
        tree_params.update(labelCol=self.get("labelCol"), featuresCol=self.get("featuresCol"),
                           predictionCol=self.get("predictionCol"))
        for i, (m, w) in enumerate(zip(self.models, self.weights)):
            mp = os.path.join(path, f"model-{i}")
            extra = {"numFeatures": int(len(self._subspace(m)))}
            if m.impurity == nat.IMPURITY_GINI:
                extra["numClasses"] = int(m.stats.shape[1])
            sp.save_metadata(mp, bl._spark_model_class, bl.uid, tree_params, bl._spark_defaults, extra)
            sp.write_tree_data(mp, m.nodes, m.stats)
            sp.write_json_row(os.path.join(path, f"data-{i}"), {"weight": w})

    @classmethod
    def _load_parts(cls, path):
        meta = sp.load_metadata(path, cls._spark_class)
        bl = _DecisionTreeEstimator.load(os.path.join(path, "learner"))
        imp = nat.IMPURITY_GINI if cls._classification else nat.IMPURITY_VARIANCE
        models, weights, nf = [], [], 0
        for i in range(int(meta["numBaseModels"])):
            mp = os.path.join(path, f"model-{i}")
            nf = max(nf, int(sp.load_metadata(mp).get("numFeatures", 0)))
            nodes, stats = sp.read_tree_data(mp)
            models.append(DecisionTreeModel(nodes, stats, imp))
            weights.append(float(sp.read_json_row(os.path.join(path, f"data-{i}"))["weight"]))
        return meta, bl, weights, models, nf

    def _finish_load(self, meta, bl, nf):
        for k, v in meta["paramMap"].items():
            if k in self._defaults:
                self._values[k] = v
        self._values["baseLearner"] = bl
        self._num_features = nf
        return self


class BoostingRegressionModel(_BoostingModel):
    """BoostingRegressionModel (BoostingRegressor.scala:373-411): the weighted mean."""

    _spark_class = "org.apache.spark.ml.regression.BoostingRegressionModel"
    _defaults = dict(_BoostingParams._defaults,
                     seed=java_string_hash("org.apache.spark.ml.regression.BoostingRegressor"))
    _validators = dict(_BoostingParams._validators,
                       loss=lambda x: str(x).lower() in REGRESSOR_LOSSES)

    def transform(self, dataset, device=0):
        """BLAS.dot(predictions, weights) / weights.sum: the dot in booster order on the device
        (sbag_predict_weighted, W_DOT with one column), the weights' left-to-right sum and the
        division here."""
        acc, n = self._weighted(dataset, device, nat.W_DOT, 1)
        acc = np.zeros(n) if acc is None else acc[:, 0]
        wsum = 0.0
        for w in self.weights:
            wsum = wsum + w
        with np.errstate(divide="ignore", invalid="ignore"):
            return acc / np.float64(wsum)

    @classmethod
    def load(cls, path):
        meta, bl, weights, models, nf = cls._load_parts(path)
        return cls(weights, models, uid=meta["uid"])._finish_load(meta, bl, nf)


class BoostingClassificationModel(_BoostingModel):
    """BoostingClassificationModel (BoostingClassifier.scala:414-447): predictRaw adds each
    booster's weight to the class it predicts; the prediction is the first argmax."""

    _spark_class = "org.apache.spark.ml.classification.BoostingClassificationModel"
    _classification = True
    _defaults = dict(_BoostingParams._defaults, rawPredictionCol="rawPrediction",
                     seed=java_string_hash("org.apache.spark.ml.classification.BoostingClassifier"))
    _validators = dict(_BoostingParams._validators,
                       loss=lambda x: str(x).lower() in CLASSIFIER_LOSSES)

    def __init__(self, num_classes, weights, models, uid=None, num_features=None):
        super().__init__(weights, models, uid, num_features)
        self.numClasses = int(num_classes)

    def predict_raw(self, dataset, device=0):
        """tmp(model.predict(features).ceil.toInt) += 1.0 * weight, in booster order, on the
        device in the pass that walks the trees (sbag_predict_weighted, W_CLASS: a gini leaf
        predicts an integral class id, and 1.0 * weight is weight)."""
        raw, n = self._weighted(dataset, device, nat.W_CLASS, self.numClasses)
        return np.zeros((n, self.numClasses)) if raw is None else raw

    def transform(self, dataset, device=0):
        """ClassificationModel.raw2prediction: rawPrediction.argmax (the first maximum)."""
        return np.argmax(self.predict_raw(dataset, device), axis=1).astype(np.float64)

    def _extra_metadata(self):
        return {"numClasses": self.numClasses, "numBaseModels": self.numBaseModels}

    @classmethod
    def load(cls, path):
        meta, bl, weights, models, nf = cls._load_parts(path)
        return cls(int(meta["numClasses"]), weights, models, uid=meta["uid"])._finish_load(meta, bl, nf)


class _BoostingEstimator(_BoostingParams):
    _base_learner_class = None

    def setBaseLearner(self, v):
        if not isinstance(v, self._base_learner_class):
            raise nat.IllegalArgumentException(
                nat.SBAG_EINVAL, f"the MI355X boosting engine fits {self._base_learner_class.__name__} "
                                 f"base learners, got {type(v).__name__}")
        return self.set("baseLearner", v)

    def setNumBaseLearners(self, v):
        return self.set("numBaseLearners", int(v))

    def setWeightCol(self, v):
        return self.set("weightCol", v)

    def setSeed(self, v):
        return self.set("seed", int(v))

    def setLoss(self, v):
        return self.set("loss", v)

    def setValidationIndicatorCol(self, v):
        return self.set("validationIndicatorCol", v)

    def setTol(self, v):
        return self.set("tol", float(v))

    def setNumRound(self, v):
        return self.set("numRound", int(v))

    def copy(self, extra=None):
        other = super().copy(extra)
        if other.get("baseLearner") is not None:
            other._values["baseLearner"] = other.get("baseLearner").copy()
        return other

    def save(self, path):
        """Boosting*Writer: Boosting*Params.saveImpl."""
        self._check_new_path(path)
        self._save_params(path)

    @classmethod
    def load(cls, path):
        meta = sp.load_metadata(path, cls._spark_class)
        est = cls(uid=meta["uid"])
        for k, v in meta["paramMap"].items():
            if k in est._defaults:
                est._values[k] = v
        est.setBaseLearner(_DecisionTreeEstimator.load(os.path.join(path, "learner")))
        return est

    def fit(self, dataset, params=None, validation=None):
        """Predictor.fit -> train.  `dataset` is a Frame or (X, y); `validation` is the boolean
        validationIndicatorCol per row, used when validationIndicatorCol is set."""
        est = self.copy(params) if params else self
        return est._train(dataset, validation)

    def _num_classes(self, y):
        return None

    def _train(self, dataset, validation):
        bl = self._base_learner()
        if self.get("weightCol"):
            warnings.warn(f"weightCol is ignored, as it is not supported by {type(bl).__name__} now.")
        frame = dataset if isinstance(dataset, Frame) else Frame(*dataset)
        X = frame.features
        if is_sparse(X):
            X = X.toarray() if hasattr(X, "toarray") else X.to_dense()
        X = np.asarray(X, np.float64)
        y = frame.label
        N, F = X.shape
        K = self._num_classes(y)
        with_validation = bool(self.get("validationIndicatorCol"))
        vmask = np.zeros(N, bool)
        if with_validation:
            if validation is None:
                raise nat.IllegalArgumentException(
                    nat.SBAG_EINVAL, "validationIndicatorCol is set but no indicator was given")
            vmask = np.asarray(validation, bool)
        part = frame.partition_offsets or [0, N]
        # a filter keeps the partitioning: the training and the validation rows of every partition
        tpart = [0] + list(np.cumsum([int((~vmask[part[p]:part[p + 1]]).sum()) for p in range(len(part) - 1)]))
        vpart = [0] + list(np.cumsum([int(vmask[part[p]:part[p + 1]].sum()) for p in range(len(part) - 1)]))
        tpart, vpart = [int(v) for v in tpart], [int(v) for v in vpart]
        Xt, yt, Xv, yv = X[~vmask], y[~vmask], X[vmask], y[vmask]
        n = len(yt)
        if n == 0:
            raise nat.SparkException(nat.SBAG_EEMPTY, "ML algorithm was given empty dataset.")
        L = self.getNumBaseLearners()
        lossf = loss_function(self.getLoss())
        classification = self._classification
        impurity = nat.IMPURITY_GINI if classification else nat.IMPURITY_VARIANCE
        agg = nat.AGG_MODE if classification else nat.AGG_MEAN
        sub = np.arange(F, dtype=np.int32)
        offs = tpart if len(tpart) > 2 else None
        ctx = nat.default_context(0)
        ds = nat.DeviceDataset.from_numpy(Xt, yt, ctx)
        try:
            w = np.ones(n)                 # boost$weight, lit(1.0)
            weights, models = [], []
            vacc = np.zeros(len(yv))       # BLAS.dot of the model so far on the validation rows
            wsum = 0.0
            it, error, num_try, seed = L, DOUBLE_MAX, 0, self.getSeed()
            while it != 0:
                proba = w / partition_sum(w, tpart)
                bag = nat.sample_boosted(ctx, proba * float(n), seed, offs)
                f = nat.fit_bag(ctx, ds, bag, sub, impurity=impurity, partition_offsets=offs,
                                max_depth=bl.getMaxDepth(), max_bins=bl.getMaxBins(),
                                min_instances_per_node=bl.getMinInstancesPerNode(),
                                min_info_gain=bl.getMinInfoGain(), tree_seed=bl.getSeed())
                try:
                    nodes, stats = f.tree(0)
                    pred = nat.predict_dataset(ctx, f, ds, agg)
                    pv = nat.predict(ctx, f, Xv, agg) if len(yv) else np.zeros(0)
                finally:
                    f.free()
                if classification:
                    ls = lossf(np.where(yt == pred, 0.0, 1.0))
                else:
                    err = np.abs(yt - pred)
                    max_error = float(err.max())
                    if max_error == 0.0:  # SQL: x / 0 is NULL, coalesced to 0.0
                        ls = np.zeros(n)
                    else:
                        ls = lossf(err / max_error)
                avgl = partition_sum(ls * proba, tpart)
                b = beta(avgl, K) if classification else beta(avgl)
                bw = weight(b)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    w = w * np.power(np.float64(b), 1 - ls)
                weights.append(bw)
                models.append(DecisionTreeModel(nodes, stats, impurity))
                if len(yv):  # evaluateOnValidation: a BoostingRegressionModel for both estimators
                    with np.errstate(invalid="ignore", over="ignore"):
                        vacc = vacc + pv * bw
                        wsum = wsum + bw
                        vpred = vacc / np.float64(wsum)
                    if classification:
                        verror = partition_sum(lossf(np.where(yv == vpred, 0.0, 1.0)), vpart)
                    else:
                        verror = partition_sum(lossf(np.abs(yv - vpred)), vpart)
                else:
                    verror = DOUBLE_MAX
                old_it = it
                it, error, num_try = terminate(avgl, with_validation, error, verror, self.getTol(),
                                               self.getNumRound(), num_try, it,
                                               float(K) if classification else 2.0)
                seed = seed + old_it
            keep = len(models) - num_try
        finally:
            ds.free()
        model = self._model(K, weights[:keep], models[:keep])
        for k in self._defaults:
            if k in model._defaults:
                model._values[k] = self.get(k)
        model._values["baseLearner"] = bl
        model._num_features = F
        return model


class BoostingRegressor(_BoostingEstimator):
    """BoostingRegressor (BoostingRegressor.scala:107-343): AdaBoost.R2 on
    DecisionTreeRegressor base learners."""

    _spark_class = "org.apache.spark.ml.regression.BoostingRegressor"
    _defaults = BoostingRegressionModel._defaults
    _validators = BoostingRegressionModel._validators
    _base_learner_class = DecisionTreeRegressor

    def _model(self, K, weights, models):
        return BoostingRegressionModel(weights, models)


class BoostingClassifier(_BoostingEstimator):
    """BoostingClassifier (BoostingClassifier.scala:109-382): SAMME on DecisionTreeClassifier
    base learners."""

    _spark_class = "org.apache.spark.ml.classification.BoostingClassifier"
    _classification = True
    _defaults = BoostingClassificationModel._defaults
    _validators = BoostingClassificationModel._validators
    _base_learner_class = DecisionTreeClassifier

    def _num_classes(self, y):
        K = int(y.max()) + 1 if len(y) else 0  # computeNumClasses: max label + 1
        if K <= 0:
            raise nat.IllegalArgumentException(
                nat.SBAG_EINVAL, f"Classifier (in extractLabeledPoints) found numClasses = {K}, "
                                 "but requires numClasses > 0.")
        bad = ~((y == np.floor(y)) & (y >= 0) & (y < K))
        if bad.any():
            raise nat.IllegalArgumentException(
                nat.SBAG_EINVAL, f"Classifier was given dataset with invalid label {y[bad][0]}.  "
                                 f"Labels must be integers in range [0, {K}).")
        return K

    def _model(self, K, weights, models):
        return BoostingClassificationModel(K, weights, models)
