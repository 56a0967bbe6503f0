/*
 * sbag.h — C ABI of the MI355X bagging engine (libsbag.so).
 *
 * Drop-in boundary for spark-ensemble's bagging hot path: BaggingRegressor /
 * BaggingClassifier `.fit` (train) and `.transform` (predict) with a
 * DecisionTree{Regressor,Classifier} base learner.  Every entry point cites the
 * reference interface it replaces (paths relative to
 * /root/reference/core/src/main/scala/org/apache/spark/).  The JNI binding a
 * maintainer adds on the Scala side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Every call returns an int status: SBAG_OK or one of the SBAG_E* codes below.
 *    The JNI shim maps SBAG_EINVAL to IllegalArgumentException (the reference's
 *    `require` / ParamValidators), SBAG_EEMPTY to SparkException ("ML algorithm
 *    was given empty dataset."), everything else to SparkException.
 *  - sbag_last_error() returns the message of the calling thread's last failure.
 *  - Host buffers passed in are read during the call only; the library owns
 *    device memory and the objects it returns until the matching *_free/_destroy.
 *  - A context is bound to one device.  Calls on one context are serialized by the
 *    library (a per-context lock): the reference runs learner Futures on a pool
 *    (ml/regression/BaggingRegressor.scala:169-191) and CrossValidator fits models
 *    concurrently, so several JVM threads may share a context.  Separate contexts
 *    run concurrently.  A dataset must be used with a context on its own device.
 */
#ifndef SBAG_H
#define SBAG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBAG_OK 0
#define SBAG_EINVAL 1       /* IllegalArgumentException (require, ParamValidators)      */
#define SBAG_EEMPTY 2       /* SparkException: empty dataset / empty subbag             */
#define SBAG_EDEVICE 3      /* HIP runtime failure                                      */
#define SBAG_ENOMEM 4       /* device allocation failure                                */
#define SBAG_EUNSUPPORTED 5 /* input outside what the engine reproduces bit-exactly     */

#define SBAG_IMPURITY_VARIANCE 0 /* DecisionTreeRegressor (impurity "variance")  */
#define SBAG_IMPURITY_GINI 1     /* DecisionTreeClassifier (impurity "gini")     */

#define SBAG_AGG_MEAN 0 /* BaggingRegressionModel.predict (BaggingRegressor.scala:248-256)      */
#define SBAG_AGG_MODE 1 /* BaggingClassificationModel.predict (BaggingClassifier.scala:248-257) */

typedef struct sbag_ctx sbag_ctx;
typedef struct sbag_dataset sbag_dataset;
typedef struct sbag_forest sbag_forest;

/* ---- contexts ---------------------------------------------------------- */
int sbag_device_count(int32_t* n);
int sbag_ctx_create(int32_t device_ordinal, sbag_ctx** out);
int sbag_ctx_destroy(sbag_ctx* ctx);
const char* sbag_last_error(void);
const char* sbag_version(void);

/* ---- sampler: bfunctions.bag (sql/bfunctions.scala:46-68) --------------
 * Multiplicities of every row for learners [learner_begin, learner_end):
 *   replacement      -> Poisson(sample_ratio) reseeded seed+i+partitionIndex
 *                       (sql/catalyst/expressions/Poisson.scala:53-56,73)
 *   !replacement, 1  -> all ones (bfunctions.scala:56-57)
 *   !replacement     -> rand(seed+i) < sample_ratio (bfunctions.scala:62-64,
 *                       Spark Rand = XORShiftRandom(seed+i+partitionIndex))
 * partition_offsets[P+1] are the Spark partition boundaries of the DataFrame
 * rows (row j of partition p gets the j-th draw of stream (i, p)).           */
typedef struct {
  int32_t replacement;  /* HasSubBag.replacement (HasSubBag.scala:39-45)            */
  int32_t pad_;
  double sample_ratio;  /* HasSubBag.sampleRatio (HasSubBag.scala:52-62)            */
  int64_t seed;         /* HasSeed.seed (default: class-name hashCode)   */
  int32_t learner_begin, learner_end; /* global learner indices                    */
} sbag_sampler_params;

int sbag_sample(sbag_ctx* ctx, const sbag_sampler_params* p, const int64_t* partition_offsets,
                int32_t num_partitions, int64_t num_rows,
                uint8_t* counts_out /* host [(end-begin) x num_rows] */);

/* ---- subspace: HasSubBag.mkSubspace (ml/ensemble/HasSubBag.scala:90-106) */
int sbag_subspace(double ratio, int32_t num_features, int64_t seed, int32_t* idx_out,
                  int32_t* n_out);

/* ---- datasets (the DataFrame's label + features columns) ---------------- */
/* X row-major [num_rows x num_features] fp64, y [num_rows]; copied to HBM as
   per-feature value codes (exact distinct-value dictionaries; u8, u16 or u32
   codes by the widest feature) + labels.                                      */
int sbag_dataset_create(sbag_ctx* ctx, int64_t num_rows, int32_t num_features, const double* X,
                        const double* y, sbag_dataset** out);
/* SparseVector rows (CSR): indptr [num_rows+1] (indptr[0] == 0), per row strictly
   increasing indices in [0, num_features), values [indptr[num_rows]]; absent entries
   are 0.0 -- Spark's SparseVector semantics, which HasSubBag.slicer
   (ml/ensemble/HasSubBag.scala:128-131) and DecisionTree see.  No dense copy is made. */
int sbag_dataset_create_csr(sbag_ctx* ctx, int64_t num_rows, int32_t num_features,
                            const int64_t* indptr, const int32_t* indices, const double* values,
                            const double* y, sbag_dataset** out);
/* Columnar features (Arrow / Parquet column chunks, or values quantized upstream):
   columns[f] points to num_rows values of type col_type.                         */
#define SBAG_COL_F64 0
#define SBAG_COL_F32 1
#define SBAG_COL_U8 2
int sbag_dataset_create_columns(sbag_ctx* ctx, int64_t num_rows, int32_t num_features,
                                int32_t col_type, const void* const* columns, const double* y,
                                sbag_dataset** out);
/* Ingest on the device: the same dataset as sbag_dataset_create / _create_columns build from
   the same arguments, byte for byte (dictionaries, zero codes, code width, row stride, zeroed
   padding columns and slack, labels), with the dictionaries discovered and the codes written by
   HIP kernels: the raw values go up in row batches (SBAG_INGEST_BATCH_ROWS lowers the batch),
   every feature's distinct values are collected in a hash set in HBM, the host sorts at most
   65 536 values a feature, and a second pass writes the codes once.  A feature with more than
   65 536 distinct values (u32 codes) takes the host ingest on the same input: the same bytes,
   and sbag_dataset_ingest_path reports SBAG_INGEST_HOST.  Errors as the host constructors'
   (a NaN anywhere: SBAG_EINVAL "NaN feature value"); after a failure nothing is returned and
   every device buffer is freed.                                                           */
#define SBAG_INGEST_HOST 0
#define SBAG_INGEST_DEVICE 1
int sbag_dataset_create_device(sbag_ctx* ctx, int64_t num_rows, int32_t num_features, const double* X,
                               const double* y, sbag_dataset** out);
int sbag_dataset_create_columns_device(sbag_ctx* ctx, int64_t num_rows, int32_t num_features,
                                       int32_t col_type, const void* const* columns, const double* y,
                                       sbag_dataset** out);
/* *path = SBAG_INGEST_DEVICE when the codes were produced by the ingest kernels, else
   SBAG_INGEST_HOST (the host constructors, import, synthetic, stacked, and a _device call that
   took the host ingest): a fallback is visible.                                            */
int sbag_dataset_ingest_path(const sbag_dataset* ds, int32_t* path);
/* Deterministic synthetic data generated directly in HBM (bench workload):
   x[r,f] = splitmix64(seed ^ (r*F+f)) mod 32; num_classes == 0 -> dyadic
   regression label, else a class label in [0, num_classes). */
int sbag_dataset_synthetic(sbag_ctx* ctx, int64_t num_rows, int32_t num_features, uint64_t seed,
                           int32_t num_classes, sbag_dataset** out);
int sbag_dataset_info(const sbag_dataset* ds, int64_t* num_rows, int32_t* num_features);
int sbag_dataset_labels(const sbag_dataset* ds, double* y_out);
int sbag_dataset_features(const sbag_dataset* ds, int64_t row_begin, int64_t row_end,
                          double* X_out /* [(row_end-row_begin) x F] */);
/* Replaces the label column (y [num_rows], host).  The reference selects whatever Double
   label column the DataFrame holds (ml/regression/BaggingRegressor.scala:146-150): labels
   that are not dyadic fixed point are fitted with Spark's row-order fp64 sums.          */
int sbag_dataset_set_labels(sbag_dataset* ds, const double* y);
/* Replication of an ingested dataset (every GPU holds the full binned matrix;
   the reference's learners share one persisted DataFrame, BaggingRegressor.scala:158-189):
   one rank ingests, exports the value codes (num_rows x row_stride x code_bytes bytes, into
   device memory of the dataset's device when codes_on_device, else host memory), the
   per-feature dictionaries (dict [dict_values], dict_off [num_features + 1]) and the labels;
   the others import them (after an RCCL broadcast of the codes, or a host copy) instead of
   re-ingesting rows.  Any of the export outputs may be NULL.  Import validates the
   dictionaries, the code width and every code on the device.                            */
int sbag_dataset_layout(const sbag_dataset* ds, int64_t* num_rows, int32_t* num_features,
                        int32_t* row_stride, int32_t* code_bytes, int64_t* dict_values);
int sbag_dataset_export(const sbag_dataset* ds, void* codes, int32_t codes_on_device, double* dict,
                        int64_t* dict_off, double* y);
int sbag_dataset_import(sbag_ctx* ctx, int64_t num_rows, int32_t num_features, int32_t row_stride,
                        int32_t code_bytes, const void* codes, int32_t codes_on_device,
                        const double* dict, const int64_t* dict_off, const double* y,
                        sbag_dataset** out);
/* datasets reference their context: free every dataset before sbag_ctx_destroy */
int sbag_dataset_free(sbag_dataset* ds);

/* ---- fit: BaggingRegressor.train / BaggingClassifier.train --------------
 * (ml/regression/BaggingRegressor.scala:121-199,
 *  ml/classification/BaggingClassifier.scala:121-199) with the base learner
 * DecisionTree{Regressor,Classifier}.fit reached through
 * HasBaseLearner.fitBaseLearner (ml/ensemble/ensembleParams.scala:99-117).     */
typedef struct {
  int32_t max_depth;              /* DecisionTree maxDepth (default 5)            */
  int32_t max_bins;               /* maxBins (default 32), 2..256                 */
  int32_t min_instances_per_node; /* default 1                                    */
  int32_t impurity;               /* SBAG_IMPURITY_*                              */
  double min_info_gain;           /* default 0.0                                  */
  int64_t seed;                   /* the base learner's seed param (HasSeed; default the
                                     class-name hashCode): seeds RandomForest.findSplits'
                                     split-finding sample of subbags > max(maxBins^2, 1e4) */
} sbag_tree_params;

typedef struct {
  sbag_sampler_params sampler;
  double subspace_ratio;       /* HasSubBag.subspaceRatio                          */
  int32_t subspace_bug_compat; /* 1: mkSubspace(getSampleRatio, ...) exactly as the
                                  reference does (BaggingRegressor.scala:174, H1)  */
  int32_t num_partitions;      /* 0 or 1 -> a single partition                    */
  const int64_t* partition_offsets; /* [num_partitions+1] or NULL                 */
  sbag_tree_params tree;
} sbag_fit_params;

int sbag_fit(sbag_ctx* ctx, sbag_dataset* ds, const sbag_fit_params* p, sbag_forest** out);

/* ---- GBM base learner: one boosting iteration's tree -----------------------
 * GBMRegressor.trainBoosters (ml/regression/GBMRegressor.scala:302-319): the subbag of
 * learner m (HasSubBag.extractSubBag of withBag's column m, HasSubBag.scala:108-126,
 * the bag drawn by sbag_sample), sliced to the booster's subspace (mkSubspace with the
 * boosting seed chain), fitted by DecisionTreeRegressor (fitBaseLearner,
 * ensembleParams.scala:99-117) on fp64 labels -- the pseudo-residuals -grad(y, F(x)).
 * Split statistics are fp64 sums in Spark's row order (DTStatsAggregator.update), so
 * trees and leaf values are those of the reference's DecisionTree on the same subbag.
 * Returns a forest of one tree (subspace = `subspace`).                           */
typedef struct {
  const uint8_t* counts;            /* host [num_rows]: the learner's bag column         */
  const int32_t* subspace;          /* the booster's feature indices, increasing          */
  int32_t subspace_len;
  int32_t num_partitions;           /* partitions of the split-finding sample (0/1: one) */
  const int64_t* partition_offsets; /* [num_partitions+1] or NULL                         */
  sbag_tree_params tree;            /* DecisionTreeRegressor params (impurity VARIANCE)   */
} sbag_booster_params;

int sbag_fit_booster(sbag_ctx* ctx, const sbag_dataset* ds, const double* labels /* host [N] */,
                     const sbag_booster_params* p, sbag_forest** out);

/* ---- Boosting (SAMME / AdaBoost.R2): the boosted bag and the base learner fit on it ----
 * BoostingParams.extractBoostedBag (ml/boosting/BoostingParams.scala:127-148): row j of
 * partition i whose prob is != 0.0 gets `new PoissonDistribution(prob)`, reseeded with
 * seed + i + j, and one sample(); the bag column BoostingClassifier.train
 * (ml/classification/BoostingClassifier.scala) and BoostingRegressor.train
 * (ml/regression/BoostingRegressor.scala) draw with prob = proba * numLines each iteration.
 * With r = partition_offsets[i] + j: counts_out[r] = 0 when mean[r] == 0.0 (nothing is
 * drawn), else the first nextPoisson(mean[r]) of a Well19937c seeded by
 * setSeed((long)(seed + i + j)) (64-bit wrapping addition), with the threshold
 * p = FastMath.exp(-mean[r]) evaluated per row on the device.  partition_offsets as in
 * sbag_sample.  SBAG_EINVAL: a negative or non-finite mean; SBAG_EUNSUPPORTED: a mean >= 40
 * (sbag_sample's limit), a draw above 255, 2^32 rows or more.  After a failure nothing has
 * been written to counts_out and the context stays usable.  num_rows == 0 is SBAG_OK.      */
int sbag_sample_boosted(sbag_ctx* ctx, const double* mean /* host [num_rows] */, int64_t seed,
                        const int64_t* partition_offsets, int32_t num_partitions,
                        int64_t num_rows, uint8_t* counts_out /* host [num_rows] */);
/* where the rows of the context's last successful sbag_sample_boosted (num_rows > 0) went */
typedef struct {
  int64_t rows_zero;     /* mean == 0.0: no draw                                              */
  int64_t rows_fast;     /* finished within fast_doubles doubles, state kept in registers     */
  int64_t rows_general;  /* ran on: second pass with the whole generator state in LDS         */
  int32_t fast_doubles;  /* nextDouble() calls the register path covers                       */
  int32_t pad_;
  double fast_ms, general_ms; /* device time of the two kernels                               */
} sbag_boosted_stats;
int sbag_sample_boosted_stats(sbag_ctx* ctx, sbag_boosted_stats* out);
/* One tree on a given bag with the dataset's own labels: the base learner fit of
 * BoostingClassifier.train (DecisionTreeClassifier, impurity GINI) and BoostingRegressor.train
 * (DecisionTreeRegressor, impurity VARIANCE) on extractBoostedBag's rows, through
 * HasBaseLearner.fitBaseLearner (ml/ensemble/ensembleParams.scala:99-117).  sbag_fit_booster
 * without a label upload: p->counts is the bag column, p->subspace the features, validation
 * and error codes are sbag_fit_booster's (an all-zero bag is SBAG_EEMPTY) plus sbag_fit's
 * label checks.  Returns a forest of one tree that carries its impurity stats (a gini tree's
 * class counts), as sbag_fit's do.                                                        */
int sbag_fit_bag(sbag_ctx* ctx, const sbag_dataset* ds, const sbag_booster_params* p,
                 sbag_forest** out);

/* ---- GBMRegressor's boosting state, resident on the device ------------------------------
 * GBMRegressor.trainBoosters (ml/regression/GBMRegressor.scala:255-399) keeps, over the rows
 * of one DataFrame, the current model's BLAS.dot S and what it derives from it every
 * iteration: on the training rows the pseudo-residuals the next booster is fitted on, on the
 * validation rows the per-row losses whose sum is the validation error.  A sbag_gbm_state is
 * bound to one resident dataset and holds, per row, y (the dataset's label column), S (fp64,
 * +0.0 at first) and `values` (fp64), all on the device; a step is one kernel (k_gbm_step).
 * With d = y - (S + konst), every operation one IEEE fp64 operation rounded to nearest, none
 * fused (GBMRegressorParams.lossFunction / gradFunction, GBMRegressor.scala:93-118):
 *   SBAG_GBM_RESIDUAL  values = -grad(y, S + konst)
 *     squared   d                                absolute  Math.signum(d): +-0.0 and NaN themselves
 *     huber     -((-d) / sqrt(1.0 + (d / alpha) * (d / alpha)))
 *     quantile  (S + konst) > y ? alpha - 1.0 : alpha
 *   SBAG_GBM_LOSS      values = lossf(y, S + konst)
 *     squared   (d * d) / 2.0                    absolute  |d|
 *     huber     (alpha * alpha) * (sqrt(1.0 + (d / alpha) * (d / alpha)) - 1.0)
 *     quantile  (S + konst) > y ? (alpha - 1.0) * d : alpha * d
 * (divisions and sqrt correctly rounded, subnormal quotients included).  NaN and infinities
 * flow through the formulas as they do on the host.
 *
 * sbag_gbm_state_create: the state over `ds` (which must outlive it), values computed for
 *   S = +0.0.  y is read from the dataset at every step: after sbag_dataset_set_labels the next
 *   step sees the new column.  SBAG_EINVAL: an unknown loss or mode, a dataset on another device than the
 *   context's; SBAG_EUNSUPPORTED: 2^32 rows or more.
 * sbag_gbm_fit_next (SBAG_GBM_RESIDUAL states): sbag_fit_booster on the state's dataset with
 *   the state's values as labels.  Nothing is uploaded and no pass analyses the labels: the
 *   step that wrote them reduced that analysis alongside.  Validation, error codes (labels
 *   not finite: SBAG_EUNSUPPORTED, "booster labels must be finite") and the returned one-tree
 *   forest are sbag_fit_booster's on the same labels, bit for bit.
 * sbag_gbm_advance: per row, p = the prediction of tree `tree_index` of `f` for the row (the
 *   tree's subspace maps its feature indices to the dataset's columns; `value <= threshold`
 *   as sbag_predict_dataset applies it, so `f` may come from another dataset: validation rows),
 *   S = S + (p * weight) with the product rounded first, then the values from the new S.
 *   SBAG_EINVAL: a tree index outside the forest, a subspace index past the dataset's features.
 * sbag_gbm_state_read: host copies of S and of the values, [num_rows] each, either may be NULL.
 * sbag_gbm_state_step_ms: device time of the state's last step kernel (create's or an advance's;
 *   0.0 for a state without rows).
 * sbag_gbm_plan: the rows one workgroup of the step owns (*tile_rows) and whether a tree of
 *   `num_nodes` nodes is staged into LDS (*tree_in_lds 1) or read from global memory (0).
 * Every call but sbag_gbm_plan holds the context as the other entries do; a context on another
 * device than the state's is SBAG_EINVAL.  After any failure the state and the context stay
 * usable.                                                                                  */
typedef struct sbag_gbm_state sbag_gbm_state;
#define SBAG_GBM_SQUARED 0
#define SBAG_GBM_ABSOLUTE 1
#define SBAG_GBM_HUBER 2
#define SBAG_GBM_QUANTILE 3
#define SBAG_GBM_RESIDUAL 0
#define SBAG_GBM_LOSS 1
int sbag_gbm_state_create(sbag_ctx* ctx, const sbag_dataset* ds, int32_t loss, double alpha,
                          double konst, int32_t mode, sbag_gbm_state** out);
int sbag_gbm_fit_next(sbag_ctx* ctx, sbag_gbm_state* state, const sbag_booster_params* p,
                      sbag_forest** out);
int sbag_gbm_advance(sbag_ctx* ctx, sbag_gbm_state* state, const sbag_forest* f, int32_t tree_index,
                     double weight);
int sbag_gbm_state_read(sbag_ctx* ctx, const sbag_gbm_state* state, double* S_out /* host [num_rows] or NULL */,
                        double* values_out /* host [num_rows] or NULL */);
int sbag_gbm_state_step_ms(sbag_ctx* ctx, const sbag_gbm_state* state, double* ms_out);
int sbag_gbm_state_free(sbag_gbm_state* state);
int sbag_gbm_plan(int32_t num_nodes, int32_t* tile_rows, int32_t* tree_in_lds);

/* ---- forest (BaggingRegressionModel / BaggingClassificationModel fields
 *      `subspaces`, `models`, `numBaseModels`, BaggingRegressor.scala:235-246) */
typedef struct { /* DecisionTreeModelReadWrite.NodeData, pre-order ids */
  int32_t id, left, right, feature; /* feature: subspace-local index, -1 for a leaf */
  int32_t split_bin, pad_;
  double threshold, prediction, impurity, gain;
} sbag_node;

int sbag_forest_num_trees(const sbag_forest* f, int32_t* n);
/* exact_splits: 1 when the tree's thresholds are Spark's (always, since the split-finding
   sample of large subbags is replayed; kept for ABI compatibility) */
int sbag_forest_tree_info(const sbag_forest* f, int32_t t, int32_t* num_nodes, int32_t* num_stats,
                          int32_t* subspace_len, int32_t* exact_splits);
int sbag_forest_subspace(const sbag_forest* f, int32_t t, int32_t* idx_out);
int sbag_forest_nodes(const sbag_forest* f, int32_t t, sbag_node* nodes_out,
                      double* stats_out /* [num_nodes x num_stats] or NULL */);
/* rebuild a forest from node arrays (model load / JNI round trip) */
int sbag_forest_create(int32_t num_trees, const int32_t* num_nodes, const sbag_node* nodes,
                       const int32_t* subspace_len, const int32_t* subspaces, int32_t impurity,
                       sbag_forest** out);
/* sbag_forest_create plus the per-node impurity stats (DecisionTreeModel's impurityStats
   column; for a gini tree the class counts of the node's rows): num_stats[t] values per node
   of tree t, concatenated [num_nodes[t] x num_stats[t]] in tree order.  Same validation as
   sbag_forest_create, and SBAG_EINVAL for a negative num_stats or a negative or non-finite
   stat.  The forest returns the stats from sbag_forest_nodes (num_stats from
   sbag_forest_tree_info), and for a gini forest its class count is the larger of
   sbag_forest_create's (largest leaf prediction + 1) and the largest num_stats.            */
int sbag_forest_create_stats(int32_t num_trees, const int32_t* num_nodes, const sbag_node* nodes,
                             const int32_t* subspace_len, const int32_t* subspaces, int32_t impurity,
                             const int32_t* num_stats /* [num_trees] */,
                             const double* stats /* concatenated [num_nodes[t] x num_stats[t]] */,
                             sbag_forest** out);
/* class count of a gini forest (the columns sbag_predict_raw fills); 0 for a variance forest */
int sbag_forest_num_classes(const sbag_forest* f, int32_t* n);
int sbag_forest_free(sbag_forest* f);

/* device-side timing of the last fit (HIP events on the context stream) */
typedef struct {
  double total_ms, sample_ms, valuecount_ms, bin_ms, compact_ms, hist_ms, split_ms, subtract_ms;
  int64_t hist_launches;
  double hist_alg_bytes;   /* Σ over hist launches: entries x (F_r + 4)   */
  double hist_entries;     /* Σ entries processed by hist launches                    */
  double hist_upper_bytes; /* SURVEY §8d upper bound: Σ_r Σ_d inbag_r x (F_r + 4) + 3N */
  int64_t levels;
  double partition_ms;     /* k_partition: rows of split nodes -> child segments      */
  double hist_work_bytes;  /* SURVEY §8d algorithmic bytes of all histograms built:
                              Σ_(r,d) n(r,d) x (F_r + 4) + 3N, n = rows of every node
                              whose histogram exists (read or obtained by subtraction) */
  double fix_ms;           /* exact-split fallback of screened variance nodes */
  int64_t exact_fallbacks; /* nodes that needed it                                      */
  double hist_lds_atomics; /* LDS atomic wave-instructions issued by the hist launches   */
  double group_ms;         /* gini class tiles: entries regrouped by tile before the
                              histogram (k_tile_count / k_tile_scatter), not in hist_ms   */
  double chain_ms;         /* fp64 labels: the chosen features' bins summed in Spark's order
                              (routing + k_fb_chainx or k_fb_psum / k_fb_pmerge) */
  double root_ms;          /* root histogram as an int8 MFMA contraction (k_hist_mfma);
                              0 when the root went through k_hist_rl (then in hist_ms)     */
  double root_mfma_ops;    /* its int8 operations (2 x 32^3 per MFMA)                      */
  int64_t hist_midrun_flushes; /* flushes of a workgroup's LDS histogram in the middle of one
                              node's run of pieces, caused by the packed word's entry limit
                              alone (0 unless one workgroup holds more than flush_limit
                              entries of a node; SBAG_HIST_FLUSH_LIMIT lowers the limit)    */
  int64_t entry_capacity;  /* per-replica stride of the fit's two in-bag entry lists: the row
                              count N (full lists), or the largest in-bag row count + 4096
                              rounded up to 64, capped at N (tight lists: real-valued labels,
                              lists past 40 % of the device, SBAG_ENT_TIGHT=1); the largest
                              of the parts of a split learner range                         */
} sbag_timing;
int sbag_forest_timing(const sbag_forest* f, sbag_timing* out);

/* ---- transform: PredictionModel.transform -> Bagging*Model.predict ------
 * slicer(subspace) (HasSubBag.scala:128-131) + tree walk + mean / breeze mode. */
int sbag_predict(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                 int32_t num_features, int32_t agg, double* out /* [num_rows] */,
                 double* per_tree_out /* [trees x num_rows] or NULL */);
int sbag_predict_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds, int32_t agg,
                         double* out /* [num_rows] */);
/* Out-of-bag predictions of a fitted ensemble on its own training data.  `ds` is the
   dataset the forest was fitted on, `sampler` and `partition_offsets` the fit's (the
   learner range must hold as many learners as the forest has trees): the bags are
   bfunctions.bag again (sbag_sample's counts; nothing is kept from the fit).  Row r is
   out of bag for learner i iff counts[i][r] == 0; n_oob[r] counts those learners and
   out[r] aggregates their trees only, in learner order:
     SBAG_AGG_MEAN  s = 0.0; s = s + tree_i(row) for every out-of-bag i; out = s / n_oob
                    (BaggingRegressor.scala:248-256 over the out-of-bag learners)
     SBAG_AGG_MODE  breeze mode of the out-of-bag votes, the first class to reach the
                    final maximum count (BaggingClassifier.scala:248-257)
   and out[r] = NaN where n_oob[r] == 0 (every row when the bags are drawn without
   replacement at ratio 1.0; not an error).  A Poisson draw above 255 fails as in a fit.
   The learners go through the device in batches when their counts exceed the budget of a
   fit's buffers; SBAG_AGG_MODE over several batches with more than 256 MB of carried
   class counters (2 x classes x num_rows bytes) is SBAG_EUNSUPPORTED. */
int sbag_predict_oob(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                     const sbag_sampler_params* sampler, const int64_t* partition_offsets,
                     int32_t num_partitions, int32_t agg, double* out /* host [num_rows] */,
                     int32_t* n_oob_out /* host [num_rows] or NULL */);
/* Out-of-bag predictions under permuted features: the device side of Breiman's permutation
   importance.  `ds`, `sampler`, `partition_offsets` and `agg` are sbag_predict_oob's (same
   validation, same error codes); base_out and n_oob_out are its out and n_oob_out, byte
   for byte.  out[k][r] is the same out-of-bag aggregation of row r (the learners with
   counts[i][r] == 0, in learner order, MEAN / MODE as above, NaN where n_oob[r] == 0) with
   one change: every tree reads feature features[k] of row r from row src_rows[k][r]; all
   other features are row r's own.  The substitution is made in the dataset's code space
   (both rows share the feature's dictionary, so it is exact); a tree whose subspace lacks
   the feature is unaffected.  src_rows[k] may be any map into [0, num_rows): a permutation,
   a shuffle within partitions or strata, a constant; the identity reproduces base_out's
   bytes.  A feature may appear in several slots, each with its own src_rows row.
   num_perm == 0 writes base_out / n_oob_out only.  SBAG_EINVAL: a feature outside
   [0, num_features), a source row outside [0, num_rows) (checked before any result is
   written; the context stays usable), num_perm < 0, or a null features / src_rows / out
   with num_perm > 0.  SBAG_EUNSUPPORTED: num_rows > INT32_MAX.
   u8 / u16 datasets whose trees fit the LDS go through one fused pass per feature batch
   (up to 64 slots, as many as the LDS holds; SBAG_OOBP_BATCH_FEATURES lowers it): a row's
   walk through a tree notes which of the batch's features it tested and walks again only
   for those, every other slot taking the baseline vote (the same bits).  Everything else
   (u32 codes, trees past the LDS chunk, more classes than the LDS counts), and every call
   under SBAG_OOBP_FORCE_FALLBACK=1, substitutes the column in a copy of the dataset's codes
   and runs a plain out-of-bag pass per slot: the same bytes, slower.  Learner batches as
   in sbag_predict_oob; SBAG_AGG_MODE over several batches carries 2 x classes x num_rows x
   (slots + 1) bytes of counters, the slots lowered to fit 256 MB and SBAG_EUNSUPPORTED when
   one slot does not. */
int sbag_predict_oob_permuted(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                              const sbag_sampler_params* sampler, const int64_t* partition_offsets,
                              int32_t num_partitions, int32_t agg,
                              const int32_t* features /* host [num_perm] global feature indices */,
                              int32_t num_perm,
                              const int32_t* src_rows /* host [num_perm x num_rows] */,
                              double* out /* host [num_perm x num_rows] */,
                              double* base_out /* host [num_rows] or NULL */,
                              int32_t* n_oob_out /* host [num_rows] or NULL */);
/* ---- staged evaluation: the score of the forest's first l + 1 trees, for every l, in one
 * pass (the out-of-bag error as a function of the number of trees: randomForest's plot(rf),
 * GBTRegressionModel.evaluateEachIteration).  out is host [trees]; stage l (0-based) is the
 * ensemble of trees [0, l].
 * With a sampler (`ds`, `sampler`, `partition_offsets` as in sbag_predict_oob: the fit's),
 * n_oob_l[r] counts the learners i <= l with counts[i][r] == 0 and pred_l[r] is
 * sbag_predict_oob's aggregation over those learners only, in learner order:
 *   SBAG_AGG_MEAN  s = 0.0; s = s + tree_i(r); pred_l = s / (double)n_oob_l
 *   SBAG_AGG_MODE  breeze's mode of the prefix's out-of-bag votes: the first class to reach
 *                  the prefix's maximum count
 * With sampler == NULL no learner is masked: every row is covered from stage 0,
 * n_oob_l = l + 1, and partition_offsets / num_partitions are ignored (the held-out curve,
 * evaluateEachIteration on a validation dataset).  y is the dataset's label column
 * (sbag_dataset_set_labels replaces it).
 * The order of the two fp64 sums is part of the interface:
 *   - per row, e = pred_l - y, se = e * e and ae = fabs(e), each rounded on its own; a row
 *     that is not covered, or that lies past num_rows, contributes +0.0;
 *   - rows fall into tiles of 512 consecutive rows, tile k holding rows [512k, 512k + 512);
 *   - a tile's 512 terms are summed by halving: for h = 256, 128, ..., 1,
 *     v[i] = v[i] + v[i + h] for i < h; the tile sum is v[0];
 *   - the stage sum starts at 0.0 and adds the tile sums in tile order, left to right;
 *   - no product or sum is contracted or reassociated;
 *   - the order does not depend on learner batches, on how the forest is staged on the
 *     device, or on which path ran.
 * covered and correct are integers: any order gives the same value.
 * Validation and error codes are sbag_predict_oob's: the sampler's learner range must hold as
 * many learners as the forest has trees, SBAG_AGG_MODE needs class-valued trees, the
 * dataset must live on the context's device and hold every feature a subspace names, a
 * Poisson draw above 255 fails as in a fit, and SBAG_AGG_MODE over several learner batches
 * with more than 256 MB of carried class counters is SBAG_EUNSUPPORTED.  A null ctx, f, ds
 * or out is SBAG_EINVAL.  num_rows == 0 is SBAG_OK with every stage zeroed.  After any
 * refusal nothing is written and the context stays usable.
 * u8 / u16 datasets whose trees fit the LDS go through one fused pass; u32 codes, trees
 * past the LDS chunk, more classes than the LDS counters hold, and every call under
 * SBAG_STAGED_FORCE_FALLBACK=1 (read on every call) take the learners' per-tree
 * predictions from the global-memory walk: the same bytes, slower.  Learner batches as in
 * sbag_predict_oob (SBAG_OOB_BATCH_LEARNERS forces their size).  Only the trees x 32 bytes
 * of out come down from the device. */
typedef struct {
  int64_t covered;  /* rows r with n_oob_l[r] >= 1                                   */
  int64_t correct;  /* SBAG_AGG_MODE: covered rows whose stage prediction == label;
                       SBAG_AGG_MEAN: 0                                              */
  double  sum_se;   /* SBAG_AGG_MEAN: sum over covered rows of e*e, e = pred_l - y;
                       SBAG_AGG_MODE: 0.0                                            */
  double  sum_ae;   /* SBAG_AGG_MEAN: sum over covered rows of |e|; MODE: 0.0        */
} sbag_stage_stats;
int sbag_eval_staged(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                     const sbag_sampler_params* sampler /* or NULL */,
                     const int64_t* partition_offsets, int32_t num_partitions, int32_t agg,
                     sbag_stage_stats* out /* host [trees] */);
/* ---- per-class raw predictions of a gini forest (ProbabilisticClassificationModel's
 * rawPrediction; neither kind is normalised).  raw_out is host [num_rows x num_classes],
 * row-major; the aggregated trees of a row are all of the forest's (sbag_predict_raw,
 * sbag_predict_raw_dataset) or its out-of-bag learners (sbag_predict_oob_raw), taken in
 * learner order.
 *   SBAG_RAW_VOTES  hard voting: raw[r][c] = the number, as an fp64 value, of the
 *                   aggregated trees whose prediction for row r is class c.  A row sums to
 *                   the tree count, or to n_oob[r].
 *   SBAG_RAW_LEAF   soft voting, RandomForestClassificationModel.predictRaw restated (the
 *                   sum of the base DecisionTreeClassificationModels' probability vectors):
 *                   s[c] = 0.0 for every class; for every aggregated tree t, with
 *                   st[0 .. ns_t) the class counts of the leaf row r reaches and
 *                   total = st[0] + st[1] + ... summed left to right: if total != 0,
 *                   s[c] = s[c] + st[c] / total for c < ns_t (classes c >= ns_t unchanged;
 *                   ns_t, the tree's num_stats, is max label + 1 of its own subbag and may be
 *                   below the forest's class count).  One tree at a time, sequential fp64.
 * Columns c >= the forest's class count (sbag_forest_num_classes) are 0.0.  num_rows == 0
 * is SBAG_OK.  SBAG_EINVAL (nothing written, the context stays usable): a null argument, an
 * unknown kind, a forest that is not gini, num_classes below the forest's class count,
 * SBAG_RAW_LEAF on a forest with a tree that carries no stats (sbag_forest_create drops
 * them; sbag_fit and sbag_forest_create_stats keep them).
 * sbag_predict_oob_raw: `ds`, `sampler` and `partition_offsets` are sbag_predict_oob's, with
 * its validation, sampler regimes, 255 cap, learner batches and error codes; row r
 * aggregates the learners i with counts[i][r] == 0, n_oob_out is sbag_predict_oob's byte
 * for byte, and a row with n_oob == 0 is a row of 0.0 (never NaN).
 * u8 / u16 codes whose trees (nodes + per-leaf payload) and classes fit the LDS go through
 * one fused pass (host rows are binned against the forest's thresholds first, in row
 * batches as in sbag_predict); everything else walks global memory, one thread per row:
 * the same bits.                                                                     */
#define SBAG_RAW_VOTES 0 /* hard voting: raw[r][c] = number of trees that predict class c     */
#define SBAG_RAW_LEAF 1  /* soft voting: raw[r][c] = in-order sum of the trees' leaf fractions */
int sbag_predict_raw(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                     int32_t num_features, int32_t kind, int32_t num_classes,
                     double* raw_out /* host [num_rows x num_classes], row-major */);
int sbag_predict_raw_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                             int32_t kind, int32_t num_classes, double* raw_out);
int sbag_predict_oob_raw(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                         const sbag_sampler_params* sampler, const int64_t* partition_offsets,
                         int32_t num_partitions, int32_t kind, int32_t num_classes,
                         double* raw_out, int32_t* n_oob_out /* host [num_rows] or NULL */);
/* ---- weighted sums over the trees: the transforms of the boosted model families.  out is
 * host [num_rows x num_cols], row-major; weights is host [num_weights], weight t that of tree
 * t; the trees are taken in forest order, one at a time, in sequential fp64.
 *   SBAG_W_DOT    (a forest of any impurity; its tree count a multiple of num_cols)
 *                 out[r][c] = 0.0 for every column; then for every tree t with
 *                 t % num_cols == c: out[r][c] = out[r][c] + (tree_t(r) * weights[t]).  The
 *                 product is rounded to fp64 before the addition: no FMA, no reassociation.
 *                 num_cols == 1 is GBMRegressionModel.predict without its `+ const`
 *                 (GBMRegressor.scala:511-516: BLAS.dot(predictions, weights)) and
 *                 BoostingRegressionModel.predict without its `/ sumWeights`
 *                 (BoostingRegressor.scala:403-405); num_cols == numClasses over trees laid
 *                 out iteration-major (tree m * numClasses + k) is the `res` of
 *                 GBMClassificationModel.predictRaw before its softmax
 *                 (GBMClassifier.scala:539-547).
 *   SBAG_W_CLASS  (a gini forest; num_cols >= sbag_forest_num_classes)
 *                 out[r][c] = 0.0 for every column; then for every tree t:
 *                 out[r][cls] = out[r][cls] + weights[t], cls the class tree_t(r) predicts.
 *                 This is BoostingClassificationModel.predictRaw
 *                 (tmp(model.predict(features).ceil.toInt) += 1.0 * weight,
 *                 BoostingClassifier.scala:428-437).  A column no tree hits stays +0.0.
 * The weights are taken as they come: negative, infinite and NaN weights follow IEEE
 * arithmetic (where a NaN comes out is defined, its payload bits are not).  The softmax, the
 * `+ const` and the `/ sumWeights` stay with the caller: one pass each over
 * num_rows x num_cols values.  num_rows == 0 is SBAG_OK.
 * SBAG_EINVAL (nothing written, the context stays usable): a null argument, an unknown kind,
 * num_weights different from the forest's tree count, num_cols < 1, SBAG_W_DOT on a tree
 * count that is no multiple of num_cols, SBAG_W_CLASS on a forest that is not gini or with
 * num_cols below its class count, a subspace that reaches past num_features (or ds's
 * features), ds on another device.
 * u8 / u16 codes whose trees fit an LDS chunk beside num_cols x 512 fp64 accumulators go
 * through one fused pass (host rows are binned against the forest's thresholds first, in row
 * batches as in sbag_predict); u32 codes, larger trees, more columns, and every call under
 * SBAG_WPRED_FORCE_FALLBACK=1 (read on every call) walk global memory, one thread per row:
 * the same bits.                                                                       */
#define SBAG_W_DOT 0   /* out[r][t % num_cols] += tree_t(r) * weights[t] */
#define SBAG_W_CLASS 1 /* out[r][class tree_t(r) predicts] += weights[t] */
int sbag_predict_weighted(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                          int32_t num_features, int32_t kind,
                          const double* weights /* host [num_weights] */, int32_t num_weights,
                          int32_t num_cols, double* out /* host [num_rows x num_cols], row-major */);
int sbag_predict_weighted_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                  int32_t kind, const double* weights, int32_t num_weights,
                                  int32_t num_cols, double* out);
/* ---- per-row quantiles across the trees of a regression forest: the spread of the ensemble
 * (prediction intervals; out of bag, their calibration).  out is host fp64
 * [num_rows x num_probs], row-major; probs is host [num_probs].
 *   Values.  For row r take the predictions of the trees concerned, -0.0 read as +0.0, sorted
 *            ascending: v[0, n).  sbag_predict_quantiles(_dataset): every tree, n = the tree
 *            count.  sbag_predict_oob_quantiles: the learners i with counts[i][r] == 0 of the
 *            sampler's bags (sbag_sample), n = n_oob[r], byte for byte sbag_predict_oob's
 *            n_oob_out.
 *   Index.   For probability p: h = (double)(n - 1) * p (one rounded product), lo = floor(h),
 *            g = h - lo.
 *   Result.  out = v[lo] when g == 0, else v[lo] + g * (v[lo + 1] - v[lo]), the subtraction,
 *            the product and the sum each rounded to fp64 on their own (no FMA).  out = NaN
 *            where n == 0.  This is NumPy's `linear` quantile up to the rounding of the
 *            interpolation, and exactly an order statistic where g == 0.
 * num_rows == 0 is SBAG_OK.
 * SBAG_EINVAL (nothing written, the context stays usable): a null argument (n_oob_out may be
 * NULL), a gini forest, num_probs outside [1, 64], a probability that is NaN or outside
 * [0, 1], a leaf that predicts NaN (hand-built forests only), and the argument errors of
 * sbag_predict / sbag_predict_dataset / sbag_predict_oob (a subspace past the features, ds on
 * another device, a sampler range that is not the forest's, bad partition offsets).
 * SBAG_EUNSUPPORTED: more than 1024 trees; for the out-of-bag call a forest whose bag counts
 * (trees x num_rows bytes) do not fit one learner batch of sbag_predict_oob (or
 * SBAG_OOB_BATCH_LEARNERS below the tree count): a row's quantile needs all its learners at
 * once.
 * A row's values are carried as ranks in the forest's dictionary of sorted distinct leaf
 * values.  u8 / u16 codes, at most 65 535 distinct leaf values, and a row tile (512, 256, 128
 * or 64 rows) whose rows, u16 rank matrix and a forest chunk fit the LDS go through one fused
 * pass that walks the trees and sorts each row's ranks in a wave (host rows are binned against
 * the forest's thresholds first, in row batches as in sbag_predict); u32 codes, more distinct
 * values, larger trees, a feature of host rows with more than 65 535 thresholds, and every
 * call under SBAG_QUANT_FORCE_FALLBACK=1 (read on every call) walk global memory, one thread
 * per row, and sort u32 ranks in a second kernel: the same bits.                          */
int sbag_predict_quantiles(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                           int32_t num_features, const double* probs /* host [num_probs] */,
                           int32_t num_probs, double* out /* host [num_rows x num_probs] */);
int sbag_predict_quantiles_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                   const double* probs, int32_t num_probs, double* out);
int sbag_predict_oob_quantiles(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                               const sbag_sampler_params* sampler, const int64_t* partition_offsets,
                               int32_t num_partitions, const double* probs, int32_t num_probs,
                               double* out, int32_t* n_oob_out /* host [num_rows] or NULL */);
/* ---- the sampling variance of a bagged prediction: the infinitesimal jackknife of Efron (2014)
 * and Wager, Hastie & Efron (2014) (ranger's se.method = "infjack", forestci), for regression
 * forests.  With c[b][i] the bag count of training row i in learner b, t_b the trees'
 * predictions of a row, m their mean, d_b = t_b - m and T trees,
 *   V_IJ = (1 / T^2) sum_i ( sum_b c[b][i] d_b )^2 = (1 / T^2) d' G d,  G[a][b] = sum_i c[a][i] c[b][i]
 * (sum_b d_b = 0: centring the counts changes nothing).  G does not depend on the row.
 *
 * The Gram matrix.  gram_out is host int64 [T x T], row-major, full and symmetric, exact:
 * gram_out[a][b] = sum_r counts[a][r] * counts[b][r].  sbag_bag_gram draws the counts of the
 * sampler's learners [learner_begin, learner_end) on the device (sbag_sample's bytes, its
 * validation and error codes; no count leaves the device); sbag_counts_gram takes counts the
 * caller kept (host u8 [T x num_rows], any byte value).  1 <= T <= 1024, else
 * SBAG_EUNSUPPORTED; sbag_bag_gram also returns SBAG_EUNSUPPORTED when the counts (T x num_rows
 * bytes) do not fit one learner batch of sbag_predict_oob (or SBAG_OOB_BATCH_LEARNERS is below
 * T).  num_rows == 0 gives zeros.  Bytes below 128 are contracted by int8 matrix instructions;
 * a count from 128 up, and every call under SBAG_GRAM_FORCE_FALLBACK=1 (read on every call),
 * takes packed-byte dot products: the same integers.
 *
 * The variance.  out is host fp64 [num_rows x 3], row-major: out[r] = { m, v_ij, v_iju }.
 * Every fp64 operation below is rounded on its own, with no FMA.
 *   - t_b is tree b's prediction of the row.  Routing is exactly sbag_predict's.
 *   - s = 0.0; s = s + t_b for b = 0..T-1, then m = s / (double)T.  These are byte for byte
 *     sbag_predict's SBAG_AGG_MEAN output.
 *   - d_b = t_b - m.
 *   - Only the diagonal and the lower triangle of gram are read.  Write
 *     Gd[a][b] = (double)gram[a][b].  An entry that is negative or >= 2^53 is SBAG_EINVAL.
 *   - Start with q = 0.0; c = 0.0;.  For a = 0..T-1:
 *       s = 0.0; and for b = 0..a-1: s = s + Gd[a][b] * d_b;
 *       u = (s + s) + Gd[a][a] * d_a;
 *       q = q + d_a * u;
 *       c = c + d_a * d_a;
 *   - v_ij = q / (double)(T * T).
 *   - On the host, in exact int64: tr = sum_a gram[a][a], tot = tr + 2 sum_{b<a} gram[a][b],
 *     w = (double)tr / (double)T - (double)tot / (double)(T * T).  A tot that overflows int64 is
 *     SBAG_EINVAL.
 *   - v_iju = v_ij - (w * c) / (double)(T * T).
 *   - Neither variance is clamped.  A negative v_iju is a legitimate Monte-Carlo outcome.
 * v_iju is the Monte-Carlo bias correction of Wager et al.: w = sum_i Var_b(c[b][i]) is the
 * empirical form of their n, right for Poisson bags of any ratio and for Bernoulli bags too.
 * SBAG_EINVAL (nothing written, the context stays usable): a null argument, a gini forest, a
 * leaf that predicts NaN, the gram errors above, and the argument errors of sbag_predict /
 * sbag_predict_dataset.  SBAG_EUNSUPPORTED: more than 1024 trees.  num_rows == 0 is SBAG_OK.
 * u8 / u16 codes and a row tile (256, 128, 64 or 32 rows) whose rows, fp64 matrix [T x rows] and
 * a forest chunk fit the LDS go through one fused pass that walks the trees and forms the
 * variance; u32 codes, larger trees, a T whose matrix fits no tile, and every call under
 * SBAG_IJ_FORCE_FALLBACK=1 (read on every call) write per-tree predictions to a workspace a row
 * batch at a time and form the variance in a second kernel: the same bits.                 */
int sbag_bag_gram(sbag_ctx* ctx, const sbag_sampler_params* sampler, const int64_t* partition_offsets,
                  int32_t num_partitions, int64_t num_rows, int64_t* gram_out /* host [T x T] */);
int sbag_counts_gram(sbag_ctx* ctx, const uint8_t* counts /* host [T x num_rows] */, int32_t T,
                     int64_t num_rows, int64_t* gram_out /* host [T x T] */);
int sbag_predict_variance(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                          int32_t num_features, const int64_t* gram /* host [T x T] */,
                          double* out /* host [num_rows x 3] */);
int sbag_predict_variance_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                  const int64_t* gram, double* out);
/* ---- partial dependence of the ensemble on one feature (randomForest's partialPlot, sklearn's
 * partial_dependence): how the prediction, averaged over the rows, moves when feature `feature`
 * (a global index) of every row is set to each of the grid's values in turn.
 * For a forest of L trees, N rows and a grid[0 .. G), finite and strictly ascending,
 * 1 <= G <= 256, define cnt[t][l][g] as the number of rows r for which tree t reaches its leaf
 * l when the tree reads grid[g] in place of the feature and row r's own value for every other
 * feature.  l counts the tree's leaves in pre-order (the order of their node ids).  A node
 * that tests the feature sends grid[g] left iff grid[g] <= threshold (Split.shouldGoLeft),
 * compared in fp64 against the node's own threshold, not through a dataset's dictionary: a grid
 * value need not be a value of the data.  A tree whose subspace lacks the feature is unaffected
 * by the substitution.  The counts are integers: any accumulation order gives the same value.
 * From the counts, in an order that is part of the interface:
 *   SBAG_PD_MEAN   (a forest of any impurity)
 *                  tree_pd[t][g] = s / (double)N, where s starts at 0.0 and adds
 *                  (double)cnt[t][l][g] * value_l for l in pre-order, each product rounded on its
 *                  own: no FMA, no reassociation.
 *                  weights == NULL: pd[g] = (in-order sum over t of tree_pd[t][g]) / (double)L,
 *                  the bagging regressor's mean (BaggingRegressor.scala:248-256).
 *                  weights != NULL: pd[g] = in-order sum over t of (tree_pd[t][g] * weights[t]),
 *                  the product rounded first: GBMRegressionModel's BLAS.dot
 *                  (GBMRegressor.scala:511-516); the caller adds `const` or divides by
 *                  sumWeights.
 *   SBAG_PD_VOTES  (a gini forest, num_classes >= sbag_forest_num_classes; weights and
 *                  per_tree_out NULL)
 *                  votes[g][c] = the integer sum over t and over the leaves l that predict class
 *                  c of cnt[t][l][g]; pd[g][c] = (double)votes[g][c] / ((double)N * (double)L).
 *                  Columns past the forest's class count are 0.0.
 * out is host [G] (MEAN) or [G x num_classes], row-major (VOTES; num_classes is ignored for
 * MEAN); per_tree_out, when given, receives tree_pd as host [trees x G].
 * SBAG_EINVAL (nothing written, the context stays usable): a null argument (weights and
 * per_tree_out may be NULL), an unknown kind, `feature` outside [0, num_features), G outside
 * [1, 256], a grid that is not finite and strictly ascending, VOTES on a forest that is not
 * gini or with num_classes below its class count, weights or per_tree_out given with VOTES,
 * num_rows == 0 (the mean of nothing), and the argument errors of sbag_predict /
 * sbag_predict_dataset (a subspace past the features, ds on another device).
 * SBAG_EUNSUPPORTED: num_rows > INT32_MAX; more than 2 GB of counts (8 bytes x the forest's
 * leaves x G).
 * With a sorted grid a row's walk through a tree splits the grid into contiguous ranges, one per
 * leaf reached, so a row costs one walk per tree, not G.  u8 / u16 codes whose trees (packed
 * nodes and int32 counters [leaves][G + 1]) fit the LDS beside a tile of 512 rows go through
 * one fused pass that keeps the counts of a tree group in LDS over a whole slice of the rows
 * (host rows are binned against the forest's thresholds first, in row batches as in
 * sbag_predict, the counts accumulating across batches); u32 codes, larger trees (or more than
 * 16 384 nodes), a tree that can hold more than 8 pending ranges at once, a feature of host rows
 * with more than 65 535 thresholds, and every call under SBAG_PD_FORCE_FALLBACK=1 (read on every
 * call) walk global memory, one thread per row: the same integers, so the same bytes.  Only out
 * and per_tree_out cross to the host.                                                       */
#define SBAG_PD_MEAN 0  /* pd[g]: the mean (or weighted sum) of the trees' mean predictions  */
#define SBAG_PD_VOTES 1 /* pd[g][c]: the fraction of (row, tree) votes for class c           */
int sbag_partial_dependence(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                            int32_t num_features, int32_t feature, const double* grid /* host [G] */,
                            int32_t G, int32_t kind, int32_t num_classes,
                            const double* weights /* host [trees] or NULL */,
                            double* out /* host [G] or [G x num_classes] */,
                            double* per_tree_out /* host [trees x G] or NULL */);
int sbag_partial_dependence_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                    int32_t feature, const double* grid, int32_t G, int32_t kind,
                                    int32_t num_classes, const double* weights, double* out,
                                    double* per_tree_out);
/* ---- per-row feature contributions: path-dependent TreeSHAP (XGBoost's pred_contribs,
 * LightGBM's predict_contrib, shap.TreeExplainer), in the per-leaf form of Lundberg's Algorithm 2.
 * out[r][g] is the contribution of global feature g to row r's prediction, out[r][num_features]
 * the bias, the ensemble's expected value; a row sums to its prediction up to rounding.  All
 * arithmetic is fp64 and every operation below is rounded on its own: no FMA, no reassociation.
 * Cover.  c(n) is stats[n][0] for a variance tree, the left-to-right sum of stats[n][0 .. ns_t)
 *   for a gini tree: the node's weighted row count, which sbag_fit, sbag_fit_bag,
 *   sbag_fit_booster and sbag_forest_create_stats keep.
 * Leaf value v_l.  class_index == -1 (a variance forest): the leaf's prediction.  class_index
 *   >= 0 (a gini forest, an index below sbag_forest_num_classes): st[class_index] / total as
 *   SBAG_RAW_LEAF, 0.0 when class_index >= ns_t.  vw_l = v_l when weights == NULL, else
 *   v_l * weights[t].
 * Paths.  For each leaf l of tree t, in pre-order, with its root-to-leaf path n_0 .. n_d:
 *   e_1 .. e_m are the distinct global features the path tests, in order of first appearance (a
 *   single-leaf tree has m = 0); z_k is the product, in path order, of c(n_{j+1}) / c(n_j) over
 *   the nodes n_j that test e_k (the first factor starts the product); o_k(r) = 1 if row r goes
 *   the path's way at every one of those nodes (left iff value <= threshold,
 *   Split.shouldGoLeft), else 0; rz_k = 1.0 / z_k; d_k = 1.0 - z_k when o_k = 1, -z_k when
 *   o_k = 0.
 * Weights.  Q(a, b) = (double)a / (double)b.  pw[0] = 1.0, every other pw 0.0.  For u = 1 .. m,
 *   with `old` the values before the step, for j = 0 .. u:
 *     pw[j] = (z_u * old[j]) * Q(u - j, u + 1), and then, only when o_u = 1 and j > 0,
 *     pw[j] = pw[j] + old[j - 1] * Q(j, u + 1).
 * Unwound sum of element k.
 *   o_k = 1: next = pw[m], total = 0.0; for i = m - 1 down to 0: tmp = next * Q(m + 1, i + 1);
 *            total = total + tmp; next = pw[i] - (tmp * z_k) * Q(m - i, m + 1).
 *   o_k = 0: total = 0.0; for i = m - 1 down to 0:
 *            total = total + (pw[i] * rz_k) * Q(m + 1, m - i).
 * Accumulation.  acc[0 .. F] starts at +0.0.  Over the trees in forest order and the leaves in
 *   pre-order: for k = 1 .. m: acc[e_k] = acc[e_k] + (total_k * d_k) * vw_l; then
 *   acc[F] = acc[F] + b, b = vw_l multiplied by z_1, z_2, .., z_m in that order.
 *   out[r][g] = acc[g] / (double)trees when weights == NULL (the bagging mean), else acc[g]: the
 *   caller adds `const` or divides by sumWeights.  A feature no tree tests is +0.0; the bias
 *   column is the same for every row.
 * SBAG_EINVAL (nothing written, the context stays usable): a null argument (weights may be
 * NULL); class_index == -1 on a gini forest, >= 0 on a variance forest, below -1 or out of
 * range; a tree without stats; a node whose cover is not finite and > 0; the argument errors of
 * sbag_predict / sbag_predict_dataset.  num_rows == 0 is SBAG_OK.  SBAG_EUNSUPPORTED: a path
 * with more than 64 distinct features; a packed path table over 2 GB (24 bytes a leaf, 40 an
 * element of a path).
 * u8 / u16 codes and forests whose paths test at most 15 distinct features go through one fused
 * pass: a lane group per (row, leaf path) with the path's permutation weights across the lanes
 * and the accumulators of a row tile in LDS (host rows are binned against the forest's thresholds
 * first, in row batches as in sbag_predict).  u32 codes, a path with more features, a feature
 * count whose 16-row tile does not fit the LDS, a feature of host rows with more than 65 535
 * thresholds and every call under SBAG_CONTRIB_FORCE_FALLBACK=1 (read on every call) take one
 * thread per row over the same path table: the same operations in the same order, so the same
 * bytes.                                                                                     */
int sbag_predict_contributions(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                               int32_t num_features, int32_t class_index,
                               const double* weights /* host [trees] or NULL */,
                               double* out /* host [num_rows x (num_features + 1)], row-major */);
int sbag_predict_contributions_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                       int32_t class_index, const double* weights, double* out);
/* ---- forest proximities (Breiman's proximity matrix, randomForest's proximity = TRUE and
 * outlier(); sklearn's apply is the first step): in how many trees two rows reach the same leaf.
 *   Leaf code.  The leaf code of (row r, tree t) is the number of leaf nodes that come before
 *               the reached leaf in tree t's pre-order node array.
 *   Routing.    The tree's subspace and the `<=` rule of sbag_predict: left iff value <=
 *               threshold, so NaN goes right and -0.0 equals +0.0.
 *   Pair count. cnt(i, j) = #{t : code_t(q_i) == code_t(r_j)} over every tree of the forest, an
 *               integer in [0, trees].  The proximity is cnt / trees; the caller divides, nothing
 *               fp64 happens on the device and no order has to be fixed: every result is one
 *               well-defined integer.
 * sbag_predict_leaves(_dataset): out is host int32 [num_rows x trees], row-major, the node id
 *   (sbag_node.id, the index in the tree's node array) of the leaf each row reaches in each tree.
 * sbag_proximity(_dataset): out is host uint16 [nq x nr], row-major, cnt(i, j) of query row i
 *   and reference row j.  The full rectangle is computed, also when both row sets are the same
 *   (the two datasets may be one object).  The query rows go in batches: neither the device
 *   buffers nor the pinned staging buffers grow with nq.
 * sbag_proximity_moments(_dataset): ref_group is host int32 [nr] with values in [0, num_groups),
 *   num_groups in [1, 16]; out is host uint64 [nq x num_groups x 2], row-major:
 *     out[i][g][0] = sum over the j with ref_group[j] == g of cnt(i, j)
 *     out[i][g][1] = sum over the j with ref_group[j] == g of cnt(i, j)^2
 *   A group without rows gives zeros.  The pair matrix never leaves the kernel.  The sums are
 *   exact: cnt <= 65 535 and nr < 2^31, so a sum of squares is below 2^63, and integer addition
 *   makes them independent of the order of accumulation.
 * nq == 0 and nr == 0 are SBAG_OK (moments of no reference rows are zeros).  A forest of either
 * impurity is accepted: a leaf is a leaf.
 * SBAG_EINVAL (nothing written, the context stays usable): a null argument, a group id outside
 * [0, num_groups), num_groups outside [1, 16], row sets whose feature counts differ, and the
 * argument errors of sbag_predict / sbag_predict_dataset (a subspace past the features, a
 * dataset on another device).  SBAG_EUNSUPPORTED: more than 65 535 trees, a tree with more than
 * 65 536 leaves, 2^31 or more reference rows.
 * Stage A writes one signature per row: the row's leaf codes, u8 when no tree has more than 256
 * leaves (code 0xFF is then a real leaf) and u16 otherwise, zero padded to a multiple of 16
 * bytes on both sides, so that cnt = trees - #{differing codes} needs no mask.  u8 / u16 feature
 * codes whose row tile (512, 256, 128 or 64 rows), signatures and a forest chunk fit the LDS go
 * through the tiled walk (host rows are binned against the forest's thresholds first, in row
 * batches as in sbag_predict); u32 codes, larger trees, a feature of host rows with more than
 * 65 535 thresholds and every call under SBAG_PROX_FORCE_FALLBACK=1 (read on every call) walk
 * global memory, one thread per row: the same signatures.  Stage B is one tiled all-pairs
 * kernel over the two signature matrices (sbag_proximity_tile: the pairs of one block), a packed
 * compare in the place of a multiply-add.
 * sbag_proximity_topk(_dataset): the k nearest reference rows of every query row; the pair
 *   matrix never leaves the kernel, nq x k entries come down.
 *   Key.        Reference rows are ordered by the key (cnt(i, j), -j): the larger count first,
 *               among equal counts the smaller j.  Keys are distinct for distinct j, so the
 *               result is one well-defined array however the work is split.
 *   Result.     idx_out is host int32 [nq x k], cnt_out host uint16 [nq x k], row-major: row i
 *               holds the k largest keys of query row i in descending order, idx_out = j and
 *               cnt_out = cnt(i, j).
 *   Self.       self_offset >= 0 leaves reference row j == i + self_offset out of query row i's
 *               candidates (queries that are rows [self_offset, self_offset + nq) of the
 *               references); an offset past nr leaves nothing out.  self_offset == -1: none.
 *   Short.      With fewer than k candidates the tail of a row is idx = -1, cnt = 0.
 *   nq == 0 is SBAG_OK; nr == 0 gives all tails.  SBAG_EINVAL (nothing written, the context
 *   stays usable): k outside [1, 64], self_offset < -1 and sbag_proximity's argument errors.
 *   SBAG_EUNSUPPORTED: what sbag_proximity refuses.  The query rows go in batches, a batch's
 *   result is 6 k bytes a row; a block of the pair kernel keeps the lists of its 128 query rows
 *   in LDS over a run of column blocks, and a second kernel merges the runs' lists
 *   (SBAG_PROX_TOPK_RUN=n, read on every call: n column blocks a run).                       */
int sbag_proximity_topk(sbag_ctx* ctx, const sbag_forest* f, const double* Xq, int64_t nq,
                        int32_t num_features_q, const double* Xr, int64_t nr, int32_t num_features_r,
                        int32_t k, int64_t self_offset, int32_t* idx_out /* host [nq x k] */,
                        uint16_t* cnt_out /* host [nq x k] */);
int sbag_proximity_topk_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* queries,
                                const sbag_dataset* references, int32_t k, int64_t self_offset,
                                int32_t* idx_out, uint16_t* cnt_out);
int sbag_proximity_tile(int32_t* block_rows, int32_t* block_cols);
int sbag_predict_leaves(sbag_ctx* ctx, const sbag_forest* f, const double* X, int64_t num_rows,
                        int32_t num_features, int32_t* out /* host [num_rows x trees] */);
int sbag_predict_leaves_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                int32_t* out);
int sbag_proximity(sbag_ctx* ctx, const sbag_forest* f, const double* Xq, int64_t nq,
                   int32_t num_features_q, const double* Xr, int64_t nr, int32_t num_features_r,
                   uint16_t* out /* host [nq x nr] */);
int sbag_proximity_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* queries,
                           const sbag_dataset* references, uint16_t* out);
int sbag_proximity_moments(sbag_ctx* ctx, const sbag_forest* f, const double* Xq, int64_t nq,
                           int32_t num_features_q, const double* Xr, int64_t nr,
                           int32_t num_features_r, const int32_t* ref_group /* host [nr] */,
                           int32_t num_groups, uint64_t* out /* host [nq x num_groups x 2] */);
int sbag_proximity_moments_dataset(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* queries,
                                   const sbag_dataset* references, const int32_t* ref_group,
                                   int32_t num_groups, uint64_t* out);
/* ---- Stacking: the level-1 dataset and the two-level transform -----------------------------
 * StackingRegressor.train (ml/regression/StackingRegressor.scala:163-171) and
 * StackingClassifier.train (ml/classification/StackingClassifier.scala:164-172) map every
 * training row to Vectors.dense(models.map(_.predict(features))) and fit the stacker on that
 * DataFrame.  sbag_dataset_create_stacked builds it on the device: `base` holds the K fitted
 * base learners (one tree each, e.g. K sbag_fit_bag trees joined by sbag_forest_create), and
 * the result is the dataset sbag_dataset_create would build from the host matrix
 * P[r][k] = tree_k(row r of ds) and ds's labels, byte for byte what sbag_dataset_export and
 * sbag_dataset_layout return for it: the same dictionaries (only values some row takes; -0.0
 * and 0.0 one value; equal predictions of different leaves one value; a leaf no row of ds
 * reaches contributes nothing), the same code width (u8 up to 256 values in the widest
 * feature, else u16), the same row_stride with zero padding columns, the same labels
 * (real-valued ones included; the new dataset owns its label images) and the same 256 bytes
 * of zero slack behind the codes.  ds need not be the data the trees were fitted on.
 * Feature k takes at most as many values as tree k has leaves, so its dictionary is the sorted
 * distinct values of the reached leaves: one pass walks the trees (in LDS chunks, any number
 * of them) writing leaf ordinals and per-leaf reached flags, the host compacts the per-tree
 * dictionaries (a few hundred doubles), a second pass maps ordinals to codes.  No array of
 * num_rows elements crosses to the host and none is sorted there.  A forest whose trees do
 * not fit an LDS chunk, a ds with u32 codes, and every call under SBAG_STACK_FORCE_FALLBACK,
 * take the host ingest (sbag_dataset_create's) fed by the per-tree predictions: the same
 * bytes, slower.
 * SBAG_EINVAL: a null argument, a subspace of `base` that reaches past ds's features, ds on
 * another device, a reached leaf that predicts NaN; SBAG_EEMPTY: as sbag_dataset_create.
 * After a failure nothing is returned and the context stays usable.                        */
int sbag_dataset_create_stacked(sbag_ctx* ctx, const sbag_dataset* ds, const sbag_forest* base,
                                sbag_dataset** out);
/* StackingRegressionModel.predict (StackingRegressor.scala:233-235) and
 * StackingClassificationModel.predict (StackingClassifier.scala:233-235):
 *   out[r] = stack.predict(Vectors.dense(models.map(_.predict(features_r))))
 * `stack` is a forest of exactly one tree whose subspace has length K = the trees of `base`;
 * its feature j is base tree subspace[j].  Anything else is SBAG_EINVAL, as is a base subspace
 * past num_features (or ds's features).  num_rows == 0 is SBAG_OK.
 * The stacker only ever compares a base prediction with a threshold, so a base leaf is packed
 * as the rank of its value among its tree's sorted distinct leaf values and a stack node as
 * the largest rank whose value is <= its threshold; the stack tree's leaf values stay fp64.
 * One fused pass walks the stack tree per row and evaluates base tree k only when a stack node
 * tests feature k (a repeated test walks the base tree again).  Host rows are binned against
 * the base forest's thresholds first, in row batches as in sbag_predict.  When the tested
 * base trees plus the stack tree do not fit the LDS, when the codes are u32, and under
 * SBAG_STACK_FORCE_FALLBACK=1, the general path runs: the ranks of all K trees into a
 * temporary [K][num_rows] buffer (chunk by chunk through the LDS, or by a node walk from
 * global memory: also SBAG_STACK_FORCE_FALLBACK=2), then the stack tree over it.  Same bits. */
int sbag_predict_stacked(sbag_ctx* ctx, const sbag_forest* base, const sbag_forest* stack,
                         const double* X, int64_t num_rows, int32_t num_features,
                         double* out /* [num_rows] */);
int sbag_predict_stacked_dataset(sbag_ctx* ctx, const sbag_forest* base, const sbag_forest* stack,
                                 const sbag_dataset* ds, double* out /* [num_rows] */);
/* ordered aggregation of per-learner predictions on the host:
   votes [num_learners x num_rows] fp64, learner order */
int sbag_aggregate(sbag_ctx* ctx, const double* votes, int32_t num_learners, int64_t num_rows,
                   int32_t agg, double* out);

/* ---- multi-GPU transform: device-resident outputs ----------
 * One process per GPU, each holding a learner shard [g*L/G, (g+1)*L/G) and the
 * replicated dataset.  The reference's aggregation is breeze's in-order sum / L
 * (BaggingRegressor.scala:248-256) and breeze mode (BaggingClassifier.scala:248-257);
 * across devices it becomes
 *   regression:      SBAG_OUT_SUM per rank (in-order sum of the shard's trees), an
 *                    RCCL all-to-all by row shard, then sbag_aggregate_device(MEAN) of
 *                    the G partial sums in rank order / L;
 *   classification:  SBAG_OUT_VOTES per rank ([trees x N] u8 / u16 class ids), an RCCL
 *                    all-to-all by row shard (rank order = learner order), then
 *                    sbag_aggregate_device(MODE) over all L votes of the shard's rows.
 * Pointers named d_* are device memory on the context's device (e.g. a torch tensor's
 * data_ptr()); both calls return after their work is complete on the device.       */
#define SBAG_OUT_SUM 2   /* fp64 [num_rows]: in-order sum of the forest's tree predictions */
#define SBAG_OUT_VOTES 3 /* [trees x num_rows] class ids, vote_bytes 1 (u8) or 2 (u16), or
                            vote_bytes 8: every tree's fp64 prediction (any impurity)  */
int sbag_predict_dataset_device(sbag_ctx* ctx, const sbag_forest* f, const sbag_dataset* ds,
                                int32_t out_kind, int32_t vote_bytes, void* d_out);
/* d_in [K x num_rows]: in_bytes 8 -> fp64 values, MEAN: out = (in-order sum of the K
   rows) / num_learners; in_bytes 1 / 2 -> u8 / u16 class ids < num_classes, MODE:
   breeze mode over the K votes in order.  d_out fp64 [num_rows].                   */
int sbag_aggregate_device(sbag_ctx* ctx, const void* d_in, int32_t in_bytes, int32_t K,
                          int64_t num_rows, int32_t agg, int32_t num_learners,
                          int32_t num_classes, double* d_out);

#ifdef __cplusplus
}
#endif
#endif
