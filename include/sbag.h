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
