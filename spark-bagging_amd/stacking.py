"""StackingRegressor / StackingClassifier and their models: the reference's Stacking family
with DecisionTree base learners and a DecisionTree stacker, the level-1 dataset built and the
two-level walk made on the device.

Mirror of (paths relative to the reference's core/src/main/scala/org/apache/spark/):

  StackingRegressor.train         ml/regression/StackingRegressor.scala:101-184
  StackingRegressionModel         ml/regression/StackingRegressor.scala:221-244
  StackingClassifier.train        ml/classification/StackingClassifier.scala:101-185
  StackingClassificationModel     ml/classification/StackingClassifier.scala:222-245
  params                          ml/stacking/StackingParams.scala, HasBaseLearners / HasStacker
                                  (ml/ensemble/ensembleParams.scala:184-287)
  persistence                     StackingRegressor.scala:49-76, 252-290 and the classifier's

fit:
  * every base learner is fitted on the whole DataFrame (fitBaseLearner): sbag_fit_bag with an
    all-ones bag, the full subspace, the learner's own tree params and seed, and the frame's
    partition offsets (they decide the split-finding sample above max(maxBins^2, 10^4) rows);
  * every row becomes Vectors.dense(models.map(_.predict(features))): the level-1 dataset,
    sbag_dataset_create_stacked -- built in device memory from the trees' leaves.  The
    reference builds it with a `map`, which keeps the partitions, so the stacker's fit gets
    the same offsets;
  * the stacker is fitted on it the same way.  For the classifier its class count is max
    label + 1 of the label column (createDataFrame drops the column metadata).
transform / predict: stack.predict(Vectors.dense(models.map(_.predict(features)))), one fused
pass (sbag_predict_stacked).

The one deliberate difference: load reads learner-$idx in index order; the reference lists the
directory, whose order Hadoop does not define.
"""
import os
import warnings

import numpy as np

from . import _native as nat
from . import persistence as sp
from .libsvm import is_sparse
from .ml import (DecisionTreeClassifier, DecisionTreeModel, DecisionTreeRegressor, Frame, Params,
                 _DecisionTreeEstimator)


class _StackingParams(Params):
    _defaults = {"baseLearners": None, "stacker": None, "parallelism": 1, "weightCol": None,
                 "labelCol": "label", "featuresCol": "features", "predictionCol": "prediction"}
    _validators = {"parallelism": lambda x: int(x) >= 1}
    _classification = False
    _learner_class = None
    _own = ("baseLearners", "stacker")  # saved as directories, not in the metadata

    def _check_learner(self, v, what):
        if not isinstance(v, self._learner_class):
            raise nat.IllegalArgumentException(
                nat.SBAG_EINVAL, f"the MI355X stacking engine fits {self._learner_class.__name__} "
                                 f"{what}, got {type(v).__name__}")
        return v

    def setBaseLearners(self, value):
        value = [self._check_learner(v, "base learners") for v in value]
        if not value:
            raise nat.IllegalArgumentException(nat.SBAG_EINVAL, "baseLearners must not be empty")
        return self.set("baseLearners", value)

    def setStacker(self, value):
        return self.set("stacker", self._check_learner(value, "stackers"))

    def setParallelism(self, value):
        return self.set("parallelism", int(value))

    def setWeightCol(self, value):
        return self.set("weightCol", value)

    def getBaseLearners(self):
        bl = self.get("baseLearners")
        if not bl:
            raise nat.IllegalArgumentException(nat.SBAG_EINVAL, "baseLearners must not be empty")
        return bl

    def getStacker(self):
        st = self.get("stacker")
        if st is None:
            raise nat.IllegalArgumentException(nat.SBAG_EINVAL, "stacker is not set")
        return st

    def getParallelism(self):
        return self.get("parallelism")

    def copy(self, extra=None):
        other = super().copy(extra)
        if other.get("baseLearners"):
            other._values["baseLearners"] = [b.copy() for b in other.get("baseLearners")]
        if other.get("stacker") is not None:
            other._values["stacker"] = other.get("stacker").copy()
        return other

    def _check_new_path(self, path):
        if os.path.exists(path):
            raise nat.IllegalArgumentException(
                nat.SBAG_EINVAL, f"Path {path} already exists. To overwrite it, please use "
                                 "write.overwrite().save(path) for Scala and use "
                                 "write().overwrite().save(path) for Java and Python.")

    def _save_params(self, path):
        """Stacking*Params.saveImpl: metadata without baseLearners and stacker, then
        learner-$idx/ (HasBaseLearners.saveImpl) and stacker/ (HasStacker.saveImpl)."""
        params = {k: v for k, v in self.extractParamMap().items() if k not in self._own and v is not None}
        defaults = {k: v for k, v in self._defaults.items() if k not in self._own and v is not None}
        sp.save_metadata(path, self._spark_class, self.uid, params, defaults)
        for i, b in enumerate(self.getBaseLearners()):
            b.save(os.path.join(path, f"learner-{i}"))
        self.getStacker().save(os.path.join(path, "stacker"))

    def _load_params(self, path):
        """Stacking*Params.loadImpl; learner-$idx in index order."""
        meta = sp.load_metadata(path, self._spark_class)
        for k, v in meta["paramMap"].items():
            if k in self._defaults and k not in self._own:
                self._values[k] = v
        learners = []
        while os.path.isdir(os.path.join(path, f"learner-{len(learners)}")):
            learners.append(_DecisionTreeEstimator.load(os.path.join(path, f"learner-{len(learners)}")))
        self.setBaseLearners(learners)
        self.setStacker(_DecisionTreeEstimator.load(os.path.join(path, "stacker")))
        return meta


def _rows(dataset):
    X = dataset.features if isinstance(dataset, Frame) else dataset
    if is_sparse(X):
        X = X.toarray() if hasattr(X, "toarray") else X.to_dense()
    X = np.asarray(X, np.float64)
    return X[None, :] if X.ndim == 1 else X


class _StackingModel(_StackingParams):
    """models and stack of Stacking*Model."""

    def __init__(self, models, stack, uid=None, num_features=None):
        super().__init__(uid)
        self.models = list(models)
        self.stack = stack
        self._num_features = int(num_features or 0)  # of the rows the base learners were fitted on
        self._forests = None

    @property
    def _impurity(self):
        return nat.IMPURITY_GINI if self._classification else nat.IMPURITY_VARIANCE

    def _subspace(self, m):
        # the base learners see every feature (the reference slices nothing here)
        nf = int(m.nodes["feature"].max()) + 1 if len(m.nodes) else 0
        return np.arange(max(nf, self._num_features, 1), dtype=np.int32)

    def native_forests(self):
        """(base forest of the K models, stack forest of one tree over K features)."""
        if self._forests is None:
            base = nat.NativeForest.from_trees([m.nodes for m in self.models],
                                               [self._subspace(m) for m in self.models], self._impurity)
            stack = nat.NativeForest.from_trees([self.stack.nodes],
                                                [np.arange(len(self.models), dtype=np.int32)], self._impurity)
            self._forests = (base, stack)
        return self._forests

    def transform(self, dataset, device=0):
        """The prediction column: a Frame, an [N x F] array, or a DeviceDataset (then without a
        copy of the rows)."""
        base, stack = self.native_forests()
        if isinstance(dataset, nat.DeviceDataset):
            return nat.predict_stacked(dataset.ctx, base, stack, dataset)
        return nat.predict_stacked(nat.default_context(device), base, stack, _rows(dataset))

    def predict(self, features):
        return float(self.transform(np.asarray(features, np.float64)[None, :])[0])

    def _save_tree(self, path, learner, m, num_features):
        tree_params = dict(learner._other_params, **learner._values)
        tree_params.update(labelCol=self.get("labelCol"), featuresCol=self.get("featuresCol"),
                           predictionCol=self.get("predictionCol"))
        extra = {"numFeatures": int(num_features)}
        if m.impurity == nat.IMPURITY_GINI:
            extra["numClasses"] = int(m.stats.shape[1])
        sp.save_metadata(path, learner._spark_model_class, learner.uid, tree_params, learner._spark_defaults,
                         extra)
        sp.write_tree_data(path, m.nodes, m.stats)

    def save(self, path):
        """Stacking*ModelWriter.saveImpl: the params, then model-$idx (the base trees) and
        stack (the stacker's tree)."""
        self._check_new_path(path)
        self._save_params(path)
        for i, (b, m) in enumerate(zip(self.getBaseLearners(), self.models)):
            self._save_tree(os.path.join(path, f"model-{i}"), b, m, len(self._subspace(m)))
        # fitBaseLearner names the level-1 columns "label" and "features"
        self._save_tree(os.path.join(path, "stack"), self.getStacker(), self.stack, len(self.models))

    @classmethod
    def load(cls, path):
        model = cls([], None)
        meta = model._load_params(path)
        model.uid = meta["uid"]
        imp = model._impurity
        nf = 0
        for i in range(len(model.getBaseLearners())):
            mp = os.path.join(path, f"model-{i}")
            nf = max(nf, int(sp.load_metadata(mp).get("numFeatures", 0)))
            model.models.append(DecisionTreeModel(*sp.read_tree_data(mp), imp))
        model.stack = DecisionTreeModel(*sp.read_tree_data(os.path.join(path, "stack")), imp)
        model._num_features = nf
        return model


class StackingRegressionModel(_StackingModel):
    """StackingRegressionModel (StackingRegressor.scala:221-244)."""

    _spark_class = "org.apache.spark.ml.regression.StackingRegressionModel"
    _learner_class = DecisionTreeRegressor


class StackingClassificationModel(_StackingModel):
    """StackingClassificationModel (StackingClassifier.scala:222-245)."""

    _spark_class = "org.apache.spark.ml.classification.StackingClassificationModel"
    _classification = True
    _learner_class = DecisionTreeClassifier


def _tree_args(learner):
    return dict(max_depth=learner.getMaxDepth(), max_bins=learner.getMaxBins(),
                min_instances_per_node=learner.getMinInstancesPerNode(),
                min_info_gain=learner.getMinInfoGain(), tree_seed=learner.getSeed())


class _StackingEstimator(_StackingParams):
    _model_class = None

    def save(self, path):
        """Stacking*Writer: Stacking*Params.saveImpl."""
        self._check_new_path(path)
        self._save_params(path)

    @classmethod
    def load(cls, path):
        est = cls()
        est.uid = est._load_params(path)["uid"]
        return est

    def fit(self, dataset, params=None):
        """Predictor.fit -> train.  `dataset` is a Frame or (X, y)."""
        est = self.copy(params) if params else self
        return est._train(dataset)

    def _check_labels(self, y):
        pass

    def _train(self, dataset):
        learners, stacker = self.getBaseLearners(), self.getStacker()
        if self.get("weightCol"):
            for b in learners:
                warnings.warn(f"weightCol is ignored, as it is not supported by {type(b).__name__} now.")
        frame = dataset if isinstance(dataset, Frame) else Frame(*dataset)
        N, F = frame.num_rows, frame.num_features
        if N == 0:
            raise nat.SparkException(nat.SBAG_EEMPTY, "ML algorithm was given empty dataset.")
        self._check_labels(frame.label)
        imp = nat.IMPURITY_GINI if self._classification else nat.IMPURITY_VARIANCE
        part = frame.partition_offsets
        offs = part if part is not None and len(part) > 2 else None
        ones = np.ones(N, np.uint8)
        ctx = nat.default_context(0)
        ds = frame.device_dataset(ctx)
        ds1 = forest = None
        try:
            models = []
            for b in learners:
                f = nat.fit_bag(ctx, ds, ones, np.arange(F, dtype=np.int32), impurity=imp,
                                partition_offsets=offs, **_tree_args(b))
                try:
                    models.append(DecisionTreeModel(*f.tree(0), imp))
                finally:
                    f.free()
            forest = nat.NativeForest.from_trees([m.nodes for m in models],
                                                 [np.arange(F, dtype=np.int32)] * len(models), imp)
            ds1 = ds.stacked(forest)
            f = nat.fit_bag(ctx, ds1, ones, np.arange(len(models), dtype=np.int32), impurity=imp,
                            partition_offsets=offs, **_tree_args(stacker))
            try:
                stack = DecisionTreeModel(*f.tree(0), imp)
            finally:
                f.free()
        finally:
            if forest is not None:
                forest.free()
            if ds1 is not None:
                ds1.free()
            ds.free()
        model = self._model_class(models, stack, num_features=F)
        for k in self._defaults:
            if k not in self._own and k in self._values:
                model._values[k] = self._values[k]
        model._values["baseLearners"] = learners
        model._values["stacker"] = stacker
        return model


class StackingRegressor(_StackingEstimator):
    """StackingRegressor (StackingRegressor.scala:80-188) on DecisionTreeRegressor base learners
    and stacker."""

    _spark_class = "org.apache.spark.ml.regression.StackingRegressor"
    _learner_class = DecisionTreeRegressor
    _model_class = StackingRegressionModel


class StackingClassifier(_StackingEstimator):
    """StackingClassifier (StackingClassifier.scala:80-189) on DecisionTreeClassifier base
    learners and stacker."""

    _spark_class = "org.apache.spark.ml.classification.StackingClassifier"
    _classification = True
    _learner_class = DecisionTreeClassifier
    _model_class = StackingClassificationModel

    def _check_labels(self, y):
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
