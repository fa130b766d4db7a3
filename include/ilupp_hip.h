/*
 * include/ilupp_hip.h -- C ABI of the MI355X-native incomplete-factorisation engine.
 *
 * Drop-in boundary for the hot path of c-f-h/ilupp: every entry point below
 * replaces one definition of the reference's pybind11 translation unit src/binding.cpp (cited per
 * function, paths relative to /root/reference).  Plain pointers and sizes only; no torch, numpy or
 * pybind types.  Indices are int32 (the reference's default `Integer`, declarations.h:49-53), values
 * fp64.
 *
 * All functions return ILUPP_OK (0) or a negative ilupp_status; ilupp_hip_last_error() gives the
 * message the reference would have thrown (same wording where the reference has one).
 *
 * Host-pointer entry points borrow the caller's buffers for the duration of the call only
 * (binding.cpp:85-89: non-owning views).  `_device` variants take pointers that already live in this
 * GPU's HBM; they are what bench.py times.
 *
 * Threads: the reference has no internal threads and no global state on this path ("Threading /
 * reentrancy"); its Python callers are single-threaded.  Here every object owns one HIP stream and its entry points are
 * serialised by the caller per object; applies of DISTINCT finished objects may run from distinct host threads.  CONSTRUCTIONS
 * (the *_create*, *_refactor* entry points) may be CALLED from several threads, but the library runs them one at a time: one
 * process-wide mutex, also across devices -- a process that drives two GPUs gets no overlap of its constructions.  The reason: their
 * work arrays come from one process-wide pool of device blocks that knows nothing of streams -- a block released while the releasing
 * object's stream still uses it is only safe to hand to work queued on that same stream or after that stream has been waited for,
 * which every construction does before it returns.  The ways to build several factorisations at once: ilupp_hip_ml_create_batch and
 * ilupp_hip_ilucp_create_batch / ilupp_hip_ilutp_create_batch (one call, many matrices, the pool's blocks partitioned per worker), or one process per GPU (bench.py --gpus N, batched.py).
 */
#ifndef ILUPP_HIP_H
#define ILUPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ilupp_precond ilupp_precond;   /* opaque; owns the factors in HBM */

typedef enum {
    ILUPP_OK = 0,
    ILUPP_ERR_INVALID = -1,        /* bad argument (binding.cpp:77-83 "matrix has size 0!", size mismatch) */
    ILUPP_ERR_WRONG_SIZE = -2,     /* binding.cpp:241-242 "vector has wrong size for preconditioner!" */
    ILUPP_ERR_ZERO_PIVOT = -3,     /* ILUT.hpp:269-270 "ILUT_heap: encountered zero pivot in row N" */
    ILUPP_ERR_NOT_TRIANGULAR = -4, /* IChol.hpp:54-55,105-107 */
    ILUPP_ERR_NO_DIAGONAL = -5,    /* ILU(0): structurally missing diagonal (reference: undefined behaviour, ILU0.hpp:39-40,64) */
    ILUPP_ERR_HIP = -6,            /* HIP runtime failure */
    ILUPP_ERR_TIMEOUT = -7,        /* dependency wait exceeded its bound (cyclic/invalid structure) */
    ILUPP_ERR_UNSUPPORTED = -8,    /* path not built yet in this round */
    ILUPP_ERR_MEMORY = -9,         /* sparse_implementation.h:3178-3179 "insufficient memory reserved" */
    ILUPP_ERR_NOT_SPD = -10,       /* ICholT: the pivot of a column is NaN (the matrix is not positive definite).  The reference has no
                                      positivity check (IChol.hpp:115-117): such a column's entries are all NaN, none passes the threshold
                                      test, the column is stored empty and its NaNs spread through the diagonals it touched.  With
                                      ILUPP_REFERENCE_NANS=1 in the environment this library returns exactly that factor instead */
    ILUPP_ERR_INTERNAL = -12,      /* an invariant of this build does not hold (a bug here, never a property of the input) */
    ILUPP_ERR_NOT_CONVERGED = -13, /* ilupp_hip_solve: binding.cpp:227 "did not converge" */
    ILUPP_ERR_DIAG_DROPPED = -11   /* ICholT: a finite pivot was dropped by the threshold or the top-k budget (dropping.hpp:8-34 does not
                                      protect it).  The reference keeps such a factor and solves with whatever entry comes first in
                                      the column; this build reports it instead (documented deviation) */
} ilupp_status;

/* binding.cpp:279  m.def("index_size") -> sizeof(Integer) */
int ilupp_hip_index_size(void);

/* message of the last failure on this thread ("" if none) */
const char *ilupp_hip_last_error(void);

/* device selection (default 0); one HIP stream per preconditioner object */
int ilupp_hip_set_device(int device);
int ilupp_hip_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Factories.  (data, indices, indptr, is_csr) exactly as the reference's make_matrix receives them
 * (binding.cpp:68-90): n = len(indptr)-1, nnz = indptr[n]; column indices sorted ascending per row
 * (the Python wrapper guarantees it, ilupp/__init__.py:70).
 * ------------------------------------------------------------------------------------------- */

/* binding.cpp:366-375  ILU0Preconditioner(data, indices, indptr, is_csr) -> GenericLUPreconditioner
 * (ILU0.hpp:69-106) */
int ilupp_hip_ilu0_create(const double *data, const int32_t *indices, const int32_t *indptr,
                          int32_t n, int is_csr, ilupp_precond **out);
int ilupp_hip_ilu0_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                 int32_t n, int is_csr, ilupp_precond **out);
/* ... for a caller that KNOWS the number of stored entries (the length of the arrays it holds -- what the reference reads as pointer[last],
 * sparse_implementation.h:3076-3089): nothing is read back before the construction starts when a matrix of this (n, nnz) was a box grid
 * before in this process (the dimensions are guessed again, grid.hip; the proof on the device covers indptr[n] == nnz and every row, and a
 * failed proof, or an (n, nnz) not seen before, takes the reading way of ilupp_hip_ilu0_create_device).  A wrong nnz is an error;
 * d_indices and d_data MUST hold at least nnz entries (the proof and the factor kernel address them with nnz as their bound before
 * indptr[n] has been compared with it). */
int ilupp_hip_ilu0_create_device_nnz(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                     int32_t n, int64_t nnz, int is_csr, ilupp_precond **out);

/* binding.cpp:299-310  ILUTPreconditioner.__init__(..., max_fill_in, threshold)  (ILUT.hpp:199-278) */
int ilupp_hip_ilut_create(const double *data, const int32_t *indices, const int32_t *indptr,
                          int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out);

/* binding.cpp:377-386  IChol0Preconditioner(...) -> GenericLLTPreconditioner (IChol.hpp:63-73) */
int ilupp_hip_ichol0_create(const double *data, const int32_t *indices, const int32_t *indptr,
                            int32_t n, int is_csr, ilupp_precond **out);

/* binding.cpp:388-397  ICholTPreconditioner(..., add_fill_in, threshold) (IChol.hpp:158-164) */
int ilupp_hip_icholt_create(const double *data, const int32_t *indices, const int32_t *indptr,
                            int32_t n, int is_csr, int32_t add_fill_in, double threshold, ilupp_precond **out);

/* SURVEY 8(f1).  binding.cpp:329-340  ILUCPreconditioner(A_data, A_indices, A_indptr, is_csr, max_fill_in, threshold)
 * -> preconditioner_implementation.h:940-958 -> ILUC2, ILUC.hpp:112-207 (Crout ILU of Li, Saad, Chow; dropping.hpp:8-34).
 * Two factors: #0 stored column-wise, #1 row-wise (binding.cpp:449-460: for COLUMN input the two are interchanged).
 * Errors: ILUPP_ERR_ZERO_PIVOT ("ILUC2: zero pivot on diagonal, k=..."), ILUPP_ERR_MEMORY (the reference's reservation of
 * min(max_fill_in n, 10 nnz) entries per factor exceeded).  The _device form borrows a matrix in HBM. */
int ilupp_hip_iluc_create(const double *data, const int32_t *indices, const int32_t *indptr,
                          int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out);
int ilupp_hip_iluc_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                 int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out);

/* The three above on a matrix that already lives in this GPU's HBM (borrowed for the duration of the call): what a
 * GPU-resident caller -- and bench.py's C3/C4 legs -- use, as ilupp_hip_ilu0_create_device does for ILU(0). */
int ilupp_hip_ilut_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                 int32_t n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out);
int ilupp_hip_ichol0_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                   int32_t n, int is_csr, ilupp_precond **out);
int ilupp_hip_icholt_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr,
                                   int32_t n, int is_csr, int32_t add_fill_in, double threshold, ilupp_precond **out);

void ilupp_hip_destroy(ilupp_precond *p);

/* ---------------------------------------------------------------------------------------------
 * Preconditioner object members (binding.cpp:233-264, wrapPreconditioner<P>)
 * ------------------------------------------------------------------------------------------- */

/* binding.cpp:237-245 apply(x): in place on a contiguous fp64 buffer of length `len` */
int ilupp_hip_apply(ilupp_precond *p, double *x, int64_t len);
/* binding.cpp:246-254 apply_trans(x) */
int ilupp_hip_apply_trans(ilupp_precond *p, double *x, int64_t len);
/* the same on a vector that already lives in HBM (asynchronous on the object's stream unless sync!=0) */
int ilupp_hip_apply_device(ilupp_precond *p, double *d_x, int64_t len, int transpose, int sync);

/* Block apply: k right-hand sides at once, X row-major n x k (row i's k values contiguous), in place; transpose != 0 applies
 * M^-T as ilupp_hip_apply_trans does.  Every column comes out bit-identical to an apply of that column alone.  Objects of the five
 * single-factorisation kinds (ILU0, ILUT, ILUC, IChol0, ICholT).  Errors: ILUPP_ERR_WRONG_SIZE ("vector has wrong size for
 * preconditioner!") for n != the dimension, ILUPP_ERR_INVALID for k < 0; k == 0 does nothing.  last_apply_ms of
 * ilupp_hip_get_timings covers the whole block apply.  No counterpart in binding.cpp (the reference applies one vector at a time). */
/* host X: staged through the device in pieces of a bounded size */
int ilupp_hip_apply_block(ilupp_precond *p, double *X, int64_t n, int64_t k, int transpose);
/* X in HBM: stream ordering and `sync` as for ilupp_hip_apply_device.  No counterpart in binding.cpp */
int ilupp_hip_apply_block_device(ilupp_precond *p, double *d_X, int64_t n, int64_t k, int transpose, int sync);
/* the route of the last block apply: "block:level" (both sweeps walk the level-ordered factors once per chunk of up to 16 columns),
 * "block:columns" (one apply per column), "" before the first one.  Measurement / test hook, no counterpart in binding.cpp */
const char *ilupp_hip_block_path(const ilupp_precond *p);

/* Stream ordering of the device-pointer entry points (*_create_device, ilupp_hip_ilu0_refactor_device,
 * ilupp_hip_apply_device).  Every object works on a private non-blocking HIP stream.  By default the caller must
 * have synchronised the producer of the device buffers before the call, and a call with sync=0 must be followed by
 * ilupp_hip_sync() before the result is read.  With a caller stream set for the calling thread (enable != 0;
 * hip_stream = the caller's hipStream_t, NULL = the legacy default stream), every such call is ordered after the work
 * already submitted to that stream, and an asynchronous apply makes that stream wait for the result. */
int ilupp_hip_set_caller_stream(void *hip_stream, int enable);

/* y = A x for a CSR matrix in HBM (row-major storage read as given; for a CSC matrix this is A^T x), on the caller's
 * stream: with ilupp_hip_apply_device the two halves of a GPU-resident Krylov iteration.  One lane per row, accumulation in
 * stored order from 0 (reference: sparse_implementation.h:2733-2760, ROW/ID branch) -- bit-identical to the reference. */
int ilupp_hip_spmv_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int64_t nnz,
                          const double *d_x, double *d_y, void *hip_stream);

/* Y = A X for a CSR matrix in HBM and a row-major block X of k columns (row i's columns at X[i * ldx .. i * ldx + k)), Y likewise
 * with leading dimension ldy, on the caller's stream.  Column j of Y is, bit for bit, ilupp_hip_spmv_device applied to column j
 * (accumulation in stored order from 0, separate multiply and add).  X and Y must not overlap (refused).  k == 0 does nothing.
 * Errors: ILUPP_ERR_INVALID for a null pointer, n <= 0, nnz < 0, k < 0, ldx < k or ldy < k -- before any launch. */
int ilupp_hip_spmm_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int64_t nnz,
                          const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int64_t k, void *hip_stream);

/* out[j] = sum_i A[i, j] * B[i, j] for j < k over two row-major blocks (leading dimensions lda, ldb), into k doubles in device memory,
 * on the caller's stream (no host read).  The reduction shape depends on n alone (min(1024, ceil(n / 256)) contiguous chunks, a fixed
 * tree inside each, a fixed order across them): column j has the bits of the same column dotted alone, on every run.  k == 0 does
 * nothing.  Errors: ILUPP_ERR_INVALID for a null pointer, n <= 0, k < 0, lda < k or ldb < k -- before any launch. */
int ilupp_hip_block_dot_device(int32_t n, int64_t k, const double *d_A, int64_t lda, const double *d_B, int64_t ldb, double *d_out,
                               void *hip_stream);

/* The masked updates of the k-column CG (ilupp_amd/device.py): contiguous row-major n x k blocks, per-column coefficients in device
 * memory, d_active[j] != 0 for the columns that move -- a column whose flag is 0 is neither read nor written.
 *   stage 0: X = X + P * coef; R = R - V * coef (V = A P)        stage 1: P = V + P * coef (V = Z; X and R unused)
 * Errors: ILUPP_ERR_INVALID for another stage, a null pointer the stage uses, n <= 0 or k < 0.  k == 0 does nothing. */
int ilupp_hip_cg_block_update_device(int32_t stage, int32_t n, int64_t k, const uint8_t *d_active, const double *d_coef, double *d_X,
                                     double *d_R, double *d_P, const double *d_V, void *hip_stream);

/* The masked updates of the k-column BiCGstab, as ilupp_hip_cg_block_update_device:
 *   stage 0: S = R - alpha AP     stage 1: Y = Y + alpha P; Y = Y + omega S; R = S - omega AS     stage 2: P = P - omega AP; P = beta P + R
 * Errors: ILUPP_ERR_INVALID for another stage, a null pointer the stage uses, n <= 0 or k < 0.  k == 0 does nothing. */
int ilupp_hip_bicgstab_block_update_device(int32_t stage, int32_t n, int64_t k, const uint8_t *d_active, const double *d_alpha,
                                           const double *d_omega, const double *d_beta, double *d_Y, double *d_R, double *d_P,
                                           double *d_S, const double *d_AP, const double *d_AS, void *hip_stream);

/* binding.cpp:255  total_nnz  (conventions per class) */
int64_t ilupp_hip_total_nnz(const ilupp_precond *p);
/* binding.cpp:257-261 */
double ilupp_hip_memory_used_calculations(const ilupp_precond *p);
double ilupp_hip_memory_allocated_calculations(const ilupp_precond *p);
double ilupp_hip_memory(const ilupp_precond *p);
int ilupp_hip_exists(const ilupp_precond *p);
const char *ilupp_hip_special_info(const ilupp_precond *p);
/* binding.cpp:262 print_info() */
void ilupp_hip_print_info(const ilupp_precond *p);
/* pre_image_dimension(), used by the size check binding.cpp:241 */
int32_t ilupp_hip_dimension(const ilupp_precond *p);

/* ---------------------------------------------------------------------------------------------
 * Factor egress (binding.cpp:118-175 wrap_matrix / wrap_all_factor_matrices -> factors_info()).
 * LU objects expose [L, U], LL^T objects [L].
 * ------------------------------------------------------------------------------------------- */
int ilupp_hip_num_factors(const ilupp_precond *p);
int ilupp_hip_factor_info(const ilupp_precond *p, int which, int32_t *rows, int32_t *cols,
                          int64_t *nnz, int *is_csr);
/* copies the factor into caller-allocated host arrays of nnz / nnz / rows+1 elements */
int ilupp_hip_factor_copy(const ilupp_precond *p, int which, double *data, int32_t *indices, int32_t *indptr);
/* device pointers of a factor (valid while p lives); for GPU-resident callers */
int ilupp_hip_factor_device_ptrs(const ilupp_precond *p, int which, const double **d_data,
                                 const int32_t **d_indices, const int32_t **d_indptr);

/* ---------------------------------------------------------------------------------------------
 * the multilevel ILU++ preconditioner, binding.cpp:284-298
 *   MultilevelILUCDPPreconditioner(A_data, A_indices, A_indptr, is_csr, iluplusplus_precond_parameter)
 *   -> multilevelILUCDPPreconditioner::make_preprocessed_multilevelILUCDP (preconditioner_implementation.h:1350-1665),
 *      apply :433-488, total_nnz preconditioner.h:312.
 * Built: BOTH factorisations of make_preprocessed_multilevelILUCDP, chosen as the reference chooses (:1376-1382):
 *   - WITHOUT pivoting (use_ILUC: PERMUTE_ROWS 0 / 1, TOTAL_PIV off, piv_tol 0 -- precon_parameter 10 of parameters_implementation.h:927-934,
 *     e.g. default_configuration(1)): matrix_sparse::partialILUC (ILUCDP.hpp:1405-2231) as a dataflow computation over all CUs;
 *   - WITH pivoting (the default-constructed parameters, default_configuration(0), (10)): matrix_sparse::partialILUCDP (:268-1404), a chain
 *     of data-dependent steps walked by one wave; many matrices at once: ilupp_hip_ml_create_batch;
 * dropping by the combined weight of the standard / error-propagation / pivot rules, the inverse-based rule (ILUPP_DROP_INVERSE;
 * precon_parameter 1, 11) and the weighted rule (ILUPP_DROP_WEIGHTED / _WEIGHTED2; precon_parameter 2, 12) -- with the last two, whose
 * estimates are recurrences over all steps, the factorisation without pivoting runs as a chain as well (working rows up to 2048 entries in LDS, up to 32768 in global memory);
 * unbounded or bounded fill; levels ended by small pivots or by the fill of L (FINAL_ROW_CRIT -1 .. 9); preprocessing steps
 * NORMALIZE_COLUMNS, NORMALIZE_ROWS, PQ_ORDERING, MAX_WEIGHTED_MATCHING_ORDERING, UNIT_OR_ZERO_DIAGONAL_SCALING, SPARSE_FIRST_ORDERING,
 * DD_SYMM_MOVE_CORNER_ORDERING_IM, SYMM_PQ (sparse_implementation.h:5214-5460) in any sequence of at most 8.  Every other parameter
 * combination (the improved Schur complement, positional dropping, FINAL_ROW_CRIT
 * < -1, an external final row) is refused with ILUPP_ERR_UNSUPPORTED: nothing is silently replaced.
 * ------------------------------------------------------------------------------------------- */
typedef struct ilupp_ml ilupp_ml;

enum {                               /* preprocessing_type values (orderings.h) this build has */
    ILUPP_PRE_NORMALIZE_COLUMNS = 1,
    ILUPP_PRE_NORMALIZE_ROWS = 2,
    ILUPP_PRE_PQ_ORDERING = 3,
    ILUPP_PRE_MAX_WEIGHTED_MATCHING_ORDERING = 4,     /* the matching itself runs on the host (sequential augmenting paths) */
    ILUPP_PRE_DD_SYMM_MOVE_CORNER_ORDERING_IM = 5,    /* refused for matrices on which the reference's own result is undefined */
    ILUPP_PRE_UNIT_OR_ZERO_DIAGONAL_SCALING = 6,
    ILUPP_PRE_SPARSE_FIRST_ORDERING = 7,
    ILUPP_PRE_SYMM_PQ = 8                             /* rows and columns by sym_ddPQ's weights (sparse_implementation.h:4926-4940, :5352-5360) */
};

enum { ILUPP_DROP_STANDARD = 1, ILUPP_DROP_STANDARD2 = 2, ILUPP_DROP_ERR_PROP = 4, ILUPP_DROP_ERR_PROP2 = 8, ILUPP_DROP_PIVOT = 16,
       ILUPP_DROP_INVERSE = 32, ILUPP_DROP_WEIGHTED = 64, ILUPP_DROP_WEIGHTED2 = 128 };   /* USE_INVERSE_DROPPING (ILUCDP.hpp:680-713, :882-916), USE_WEIGHTED_DROPPING[2]
                                       (:629-631, :670-674): estimates that accumulate over the steps in their order -- the factorisation runs as a chain */

typedef struct {                     /* the fields of iluplusplus_precond_parameter (parameters.h:120-235) the built family reads */
    double threshold;                /* threshold */
    int32_t n_preprocessing;         /* PREPROCESSING: number of steps, */
    int32_t preprocessing[8];        /*                the steps (ILUPP_PRE_*) */
    double pq_threshold;             /* PQ_THRESHOLD */
    int32_t max_levels;              /* MAX_LEVELS */
    int32_t min_ml_size;             /* MIN_ML_SIZE */
    int32_t small_pivot_terminates;  /* SMALL_PIVOT_TERMINATES */
    double min_pivot;                /* MIN_PIVOT */
    double min_elim_factor;          /* MIN_ELIM_FACTOR */
    double threshold_shift_schur;    /* THRESHOLD_SHIFT_SCHUR */
    double vary_threshold_factor;    /* VARY_THRESHOLD_FACTOR */
    int32_t use_final_threshold;     /* USE_FINAL_THRESHOLD */
    double final_threshold;          /* FINAL_THRESHOLD */
    int32_t max_fill_in;             /* 0: MAX_FILLIN_IS_INF; else fill_in (entries a row of U / a column of L may have, the 1 included) */
    int32_t drop_rules;              /* ILUPP_DROP_*: USE_STANDARD_DROPPING, _DROPPING2, USE_ERR_PROP_DROPPING, _DROPPING2, USE_PIVOT_DROPPING */
    double weight_standard_drop, weight_standard_drop2, weight_err_prop_drop, weight_err_prop_drop2, weight_pivot_drop;   /* WEIGHT_* */
    int32_t combine_factor;          /* COMBINE_FACTOR */
    double neutral_element, min_weight;   /* NEUTRAL_ELEMENT, MIN_WEIGHT */
    int32_t scale_weight_invdiag;    /* SCALE_WEIGHT_INVDIAG */
    /* the factorisation WITH pivoting (reference partialILUCDP, ILUCDP.hpp:268-1404) is taken unless PERMUTE_ROWS is 0 or 1, total pivoting
     * is off (BEGIN_TOTAL_PIV 0 or TOTAL_PIV 0) and piv_tol is 0 (preconditioner_implementation.h:1376-1382): the reference's
     * default-constructed parameters select it */
    double piv_tol;                      /* piv_tol */
    int32_t permute_rows;                /* PERMUTE_ROWS 0..3 */
    int32_t total_piv;                   /* TOTAL_PIV 0..2 */
    int32_t begin_total_piv;             /* BEGIN_TOTAL_PIV */
    int32_t final_row_crit;              /* FINAL_ROW_CRIT -1..9 */
    double move_level_factor;            /* MOVE_LEVEL_FACTOR */
    double row_u_max;                    /* ROW_U_MAX */
    double weight_inverse_drop;          /* WEIGHT_INVERSE_DROP (with ILUPP_DROP_INVERSE) */
    double weight_weighted_drop;         /* WEIGHT_WEIGHTED_DROP (with ILUPP_DROP_WEIGHTED) */
    double init_weights_lu;              /* INIT_WEIGHTS_LU */
} ilupp_ml_params;

/* default_configuration(1) (parameters_implementation.h:546-549: set_PQ + precon_parameter 10) with threshold 0 */
void ilupp_hip_ml_default_params(ilupp_ml_params *p);
int ilupp_hip_ml_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr,
                        const ilupp_ml_params *params, ilupp_ml **out);
int ilupp_hip_ml_create_device(const double *d_data, const int32_t *d_indices, const int32_t *d_indptr, int32_t n, int is_csr,
                               const ilupp_ml_params *params, ilupp_ml **out);
/* BASELINE config 5's batched shape: `count` independent matrices (host arrays, all CSR or all CSC), one preconditioner each -- what a
 * caller of the reference does by calling the constructor once per matrix (preconditioner_implementation.h:1483-1494 runs once per
 * matrix).  The constructions run side by side (one host thread and HIP stream per matrix, at most ILUPP_BATCH_WORKERS = 64 at a
 * time), and the sequential chains of the factorisation with pivoting -- one wave each -- are launched TOGETHER, one workgroup per
 * matrix, so that a batch costs about what its slowest member costs.  out[i] / status[i] per matrix (status may be NULL); returns the
 * first error.  Every result is identical to what ilupp_hip_ml_create gives for that matrix. */
int ilupp_hip_ml_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr, const int32_t *n,
                              int is_csr, const ilupp_ml_params *params, ilupp_ml **out, int32_t *status);
void ilupp_hip_ml_destroy(ilupp_ml *p);
/* binding.cpp:237-254 apply / apply_trans, in place on a host vector; the _device form on a vector in HBM (sync as above) */
int ilupp_hip_ml_apply(ilupp_ml *p, double *x, int64_t len, int transpose);
int ilupp_hip_ml_apply_device(ilupp_ml *p, double *d_x, int64_t len, int transpose, int sync);
/* one half of the split preconditioner on a vector in HBM: apply_preconditioner_left / _right (preconditioner_implementation.h:441-453,
 * :468-486), what the reference's solver loop uses with SPLIT preconditioning (solving_routines_implementation.h:81); left != 0: the left part */
int ilupp_hip_ml_apply_part_device(ilupp_ml *p, double *d_x, int64_t len, int transpose, int left, int sync);
/* Many multilevel objects (each at most once) applied at once: member i's vector is d_x + offsets[i] (offsets: a host array of `count`
 * entries, in doubles), of length n_i, in place; what lies between the vectors is left untouched.  ONE launch for all members whose n fits
 * the kernel's LDS cap (one workgroup per member, which walks the member's levels up and down as the single apply does -- scale / permute,
 * one sweep with the unknowns in LDS, take / permute, on the last n_level entries of the vector -- k_ml_apply_batch, sptrsv_batch.hip); a
 * member that is too large (route 1: for the cap, or, with n > 4096, for a launch it would have to itself) or one of whose level objects
 * has a factor with an empty row (route 2) goes through ilupp_hip_ml_apply_device's path inside the same call, so the call succeeds
 * wherever the loop of single applies would.  route (may be NULL) receives 0, 1 or 2 per member.  Every result has the bits of
 * ilupp_hip_ml_apply_device.  Ordered on the caller's stream; sync == 0 returns without waiting (and without reading the members' error
 * words), sync != 0 waits and reports a member whose sweep gave up as ILUPP_ERR_TIMEOUT, "member i of the batch: triangular solve:
 * dependency wait timed out ..." (that member's vector is unspecified, the other members' vectors are complete).  A later single apply or
 * the destruction of a member is queued behind a launch that was not waited for.  ILUPP_BATCH_APPLY_MAX_N (read on every call) lowers the
 * cap.  Refused with ILUPP_ERR_INVALID before any device call: null lists or members, a negative count, a member that is not a live
 * multilevel object, a member named twice.  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_ml_apply_batch_device(int32_t count, ilupp_ml *const *members, double *d_x, const int64_t *offsets, int transpose, int sync,
                                    int32_t *route);
/* The same on host vectors x[i] of len[i] == n_i doubles, in place: all vectors staged through one device buffer (one packed upload, one
 * download); waits for the result.  A member that failed keeps its vector as it was. */
int ilupp_hip_ml_apply_batch(int32_t count, ilupp_ml *const *members, double *const *x, const int64_t *len, int transpose, int32_t *route);
/* the largest n that takes route 0 of the two entries above on the current device (what the device gives a workgroup of k_ml_apply_batch
 * in LDS, ILUPP_BATCH_APPLY_MAX_N applied); negative: an error code */
int64_t ilupp_hip_ml_apply_batch_max_n(void);
int ilupp_hip_ml_sync(ilupp_ml *p);
/* levels() (preconditioner.h:298), total_nnz (:312), dim(k) */
int32_t ilupp_hip_ml_levels(const ilupp_ml *p);
int64_t ilupp_hip_ml_total_nnz(const ilupp_ml *p);
/* one level (extract_left_matrix(k) ... extract_right_scaling(k), preconditioner.h:288-296): sizes, then copies to host buffers
 * (any pointer may be NULL): L by columns, U by rows (data / indices of nnz entries, indptr of n + 1), the middle diagonal,
 * the four permutations and the two scalings, n entries each */
int ilupp_hip_ml_level_info(const ilupp_ml *p, int32_t level, int32_t *n, int64_t *nnz_left, int64_t *nnz_right);
int ilupp_hip_ml_level_copy(const ilupp_ml *p, int32_t level, double *l_data, int32_t *l_indices, int32_t *l_indptr, double *u_data,
                            int32_t *u_indices, int32_t *u_indptr, double *middle, int32_t *perm_rows, int32_t *perm_cols,
                            int32_t *inv_perm_rows, int32_t *inv_perm_cols, double *d_left, double *d_right);
/* GPU milliseconds of the construction (whole, and the factorisation kernels alone) and of the last apply */
int ilupp_hip_ml_timings(const ilupp_ml *p, float *construct_ms, float *kernel_ms, float *last_apply_ms);

/* _ilupp.solve (binding.cpp:200-230, bound at :281): the multilevel preconditioner of `params` is built for A, then BiCGstab with SPLIT
 * preconditioning runs from the zero vector (solve_with_multilevel_preconditioner, solving_routines_implementation.h:81 -> bicgstab,
 * iterative_solvers_implementation.h:385-530) until res / initial_res <= rtol and res <= atol, or max_iter iterations (at least one).
 * A, rhs and x are host arrays (x: n doubles, written in every case that reaches the iteration); the matrix, the preconditioner and
 * every vector of the iteration live in HBM, the host sees one residual norm per iteration.  *iterations, *rel_reached (res /
 * initial_res) and *abs_reached (res) are what the reference returns as (max_iter, 10^-rel_tol, 10^-abs_tol).
 * Returns ILUPP_ERR_NOT_CONVERGED where the reference throws "did not converge", ILUPP_ERR_WRONG_SIZE for "right-hand side has wrong
 * size!" (:209-210), and the errors of ilupp_hip_ml_create. */
int ilupp_hip_solve(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, const double *rhs, int64_t rhs_len,
                    double rtol, double atol, int32_t max_iter, const ilupp_ml_params *params, double *x, int32_t *iterations, double *rel_reached,
                    double *abs_reached);

/* ---------------------------------------------------------------------------------------------
 * ILUCP: Crout ILU with column pivoting.  Replaces binding.cpp:343-356 (ILUCPPreconditioner.__init__ ->
 * preconditioner_implementation.h:1117-1147 -> ILUCP4, ILUC.hpp:212-370) and its apply (triangular_solve_perm,
 * sparse_implementation.h:4166-4253).  A chain of n data-dependent steps: one wave of the GPU walks it (ilucp.hip); many matrices at
 * once: ilupp_hip_ilucp_create_batch.
 * Errors: ILUPP_ERR_MEMORY ("ILUCP4: Insufficient memory reserved. Increase mem_factor", ILUC.hpp:287-289, :344-346).
 * ------------------------------------------------------------------------------------------- */
typedef struct ilupp_ilucp ilupp_ilucp;
int ilupp_hip_ilucp_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, int32_t max_fill_in,
                           double threshold, double piv_tol, int32_t row_pos, double mem_factor, ilupp_ilucp **out);
void ilupp_hip_ilucp_destroy(ilupp_ilucp *p);
/* binding.cpp:237-254 apply / apply_trans, in place on a host vector */
int ilupp_hip_ilucp_apply(ilupp_ilucp *p, double *x, int64_t len, int transpose);
int64_t ilupp_hip_ilucp_total_nnz(const ilupp_ilucp *p);
int32_t ilupp_hip_ilucp_zero_pivots(const ilupp_ilucp *p);
/* the factors as ILUCP4 returns them for the major-order view of the input (L by columns with its 1 first; U by rows with the pivot first
 * and the original column indices) and the permutation (binding.cpp:178-196 permutations(): the right one for COLUMN input, the left one
 * for ROW input); any pointer may be NULL */
int ilupp_hip_ilucp_info(const ilupp_ilucp *p, int32_t *n, int64_t *nnz_l, int64_t *nnz_u, float *kernel_ms);
int ilupp_hip_ilucp_copy(const ilupp_ilucp *p, double *l_data, int32_t *l_indices, int32_t *l_indptr, double *u_data, int32_t *u_indices,
                         int32_t *u_indptr, int32_t *perm);

/* ILUTP: ILUT with column pivoting.  Replaces binding.cpp:313-326 (ILUTPPreconditioner.__init__ -> preconditioner_implementation.h:1050-1078 ->
 * ILUTP2, ILUTP.hpp:13-140).  The object is of the same type as ILUCP's and shares its apply / total_nnz / info / copy / destroy entry points;
 * its factors belong to the ROWS of the view: L by rows (its 1 last, columns in the permuted numbering), U by rows (the pivot first, original
 * column indices, ordered by permuted position).  Errors: ILUPP_ERR_MEMORY ("ILUTP2: memory reserved was insufficient."), ILUPP_ERR_ZERO_PIVOT
 * ("matrix_sparse::ILUTP2: encountered zero pivot in row N") */
int ilupp_hip_ilutp_create(const double *data, const int32_t *indices, const int32_t *indptr, int32_t n, int is_csr, int32_t max_fill_in,
                           double threshold, double piv_tol, int32_t row_pos, double mem_factor, ilupp_ilucp **out);
/* Many matrices at once, with the contract of ilupp_hip_ml_create_batch: `count` independent matrices (host arrays, all CSR or all CSC),
 * one parameter set, one preconditioner each.  The constructions run side by side (one host thread and HIP stream per matrix, at most
 * ILUPP_BATCH_WORKERS = 64 at a time, fewer if the device memory takes fewer), and their chains -- one wave each -- are launched TOGETHER,
 * one workgroup per matrix, so that a batch's chains cost about what its slowest member's costs (64 chains of n = 12000: 1.0 - 1.3 x one,
 * profiles/r09_pivot_batch.txt); kernel_ms of a member is that combined launch's time.  out[i] is NULL and status[i] the code of a member that failed (status may be NULL); members are independent, one
 * failing does not stop the others; returns the first error, whose message starts "matrix i of the batch: ".  count == 0 returns
 * ILUPP_OK without touching the device.  Every result is identical to what ilupp_hip_ilucp_create / ilupp_hip_ilutp_create gives for
 * that matrix. */
int ilupp_hip_ilucp_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                 const int32_t *n, int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos,
                                 double mem_factor, ilupp_ilucp **out, int32_t *status);
int ilupp_hip_ilutp_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                 const int32_t *n, int is_csr, int32_t max_fill_in, double threshold, double piv_tol, int32_t row_pos,
                                 double mem_factor, ilupp_ilucp **out, int32_t *status);

/* The single apply of an ILUCP / ILUTP object in place on a DEVICE vector of `len` doubles (both classes share the handle type), ordered on
 * the caller's stream like ilupp_hip_apply_device: behind the work submitted to it so far, and with sync == 0 the caller's stream waits for
 * the result instead of the host. */
int ilupp_hip_ilucp_apply_device(ilupp_ilucp *p, double *d_x, int64_t len, int transpose, int sync);
/* Many ILUCP / ILUTP objects (mixed at will, each at most once) applied at once: member i's vector is d_x + offsets[i] (offsets: a host
 * array of `count` entries, in doubles), of length n_i, in place; what lies between the vectors is left untouched.  ONE launch for all
 * members whose n fits the kernel's LDS cap (one workgroup per member: the permutation and both sweeps of the apply inside it, the unknowns
 * in LDS -- k_pivot_apply_batch, sptrsv_batch.hip); a member that is too large (route 1: for the cap, or, with n > 4096, for a launch it
 * would have to itself -- one workgroup is slower there than the single apply's sweeps) or whose factors have an empty row (route 2) goes
 * through the single apply inside the same call, so the call succeeds wherever the loop of single applies would.  route (may be NULL)
 * receives 0, 1 or 2 per member.  Every result has the bits of ilupp_hip_ilucp_apply.  Ordered on the caller's stream; sync == 0 returns
 * without waiting (and without reading the members' error words), sync != 0 waits and reports a member whose sweep gave up as
 * ILUPP_ERR_TIMEOUT, "member i of the batch: triangular solve: dependency wait timed out ..."; the other members' vectors are complete.
 * ILUPP_BATCH_APPLY_MAX_N (read on every call) lowers the cap.  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_pivot_apply_batch_device(int32_t count, ilupp_ilucp *const *members, double *d_x, const int64_t *offsets, int transpose, int sync,
                                       int32_t *route);
/* The same on host vectors x[i] of len[i] == n_i doubles, in place: all vectors staged through one device buffer (one packed upload, one
 * download); waits for the result.  A member that failed keeps its vector as it was. */
int ilupp_hip_pivot_apply_batch(int32_t count, ilupp_ilucp *const *members, double *const *x, const int64_t *len, int transpose, int32_t *route);
/* Left-preconditioned BiCGstab for MANY small systems at once, each with its own ILUCP / ILUTP object (mixed at will, each at most once):
 * ONE launch, one workgroup per system, which runs the whole loop on the device -- SpMV, apply, dot products, updates and the convergence
 * test (k_bicgstab_batch, sptrsv_batch.hip) -- with no host round trip.  Member i: the CSR matrix d_data[i] / d_indices[i] /
 * d_indptr[i] (device arrays; n_i = the object's n, nnz[i] entries; the four lists are host arrays), the right-hand side d_b + offsets[i],
 * the start d_x0 + offsets[i] (d_x0 may be NULL: zero) and the result d_x + offsets[i], n_i doubles each; what lies between the vectors
 * of d_x is left untouched.  d_work: 7 * sum n_i doubles of device memory (work_doubles says how many there are).  The loop is that of
 * ilupp_amd.device.bicgstab for one column: at most maxiter iterations; every check_every iterations (0: never), when rtol > 0, a member
 * whose ||r|| / ||r_0|| (preconditioned residuals) is at or below rtol stops as converged; a zero right-hand side or initial residual:
 * converged at once, x = x0; rho, (Ap, r0*) or omega zero or not finite: the member stops, not converged.  Per member (device arrays of
 * `count`): d_iterations, d_flags (bit 0: still active after maxiter iterations, 1: converged, 2: a sweep gave up -- x untouched, 3: zero
 * right-hand side or initial residual), d_rr = (r, r) at exit and d_init = ||r_0||.  Every member has the bits of the same solve done alone
 * with ilupp_hip_spmv_device, ilupp_hip_ilucp_apply_device, ilupp_hip_block_dot_device and ilupp_hip_bicgstab_block_update_device.
 * route (may be NULL): 0 = solved in the launch; 1 = n above the launch's LDS cap (the apply's cap less the dot scratch;
 * ILUPP_BATCH_APPLY_MAX_N lowers it); 2 = degenerate factor: members of routes 1 and 2 are NOT solved, their vectors and output words are
 * left untouched -- the caller solves them one by one.  A lone member also takes the launch (measured
 * faster than its single solve at n = 1 000 and 4 000: profiles/r11_pivot_bicgstab_batch.txt).  Ordered on the caller's stream; sync == 0
 * returns without waiting, sync != 0 waits and reports a member whose sweep gave up as ILUPP_ERR_TIMEOUT.  Refused with ILUPP_ERR_INVALID
 * before any device call: null lists or members, a negative count, maxiter or check_every, a member named twice, a workspace that is too
 * small.  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_pivot_bicgstab_batch_device(int32_t count, ilupp_ilucp *const *members, const double *const *d_data, const int32_t *const *d_indices,
                                          const int32_t *const *d_indptr, const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x,
                                          const int64_t *offsets, double *d_work, int64_t work_doubles, int32_t maxiter, double rtol,
                                          int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync,
                                          int32_t *route);
/* the largest n that takes route 0 on the current device (what the device gives a workgroup in LDS, ILUPP_BATCH_APPLY_MAX_N applied);
 * negative: an error code */
int64_t ilupp_hip_pivot_apply_batch_max_n(void);
/* The batched apply for the NON-pivoting classes: many ILU0 / ILUT / ILUC / IChol0 / ICholT objects (mixed at will, each at most once)
 * applied at once by the same launch (k_pivot_apply_batch on descriptors without a permutation).  Arguments, routes, ordering, sync and
 * ILUPP_BATCH_APPLY_MAX_N as for ilupp_hip_pivot_apply_batch_device; members of routes 1 and 2 go through ilupp_hip_apply_device's path
 * inside the call.  Every result has the bits of ilupp_hip_apply_device, whichever route that single apply takes (a member whose single
 * apply runs a static form is swept from its CSR triangles here; the launch never starts a static analysis).  A re-factorisation
 * (ilupp_hip_ilu0_refactor_device) or the destruction of a member is queued behind a launch that was not waited for.  Refused with
 * ILUPP_ERR_INVALID before any device call: null lists or members, a negative count, a member named twice ("a preconditioner appears
 * twice in the batch"), a multilevel handle.  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_apply_batch_device(int32_t count, ilupp_precond *const *members, double *d_x, const int64_t *offsets, int transpose, int sync,
                                 int32_t *route);
/* Preconditioned conjugate gradients for MANY small symmetric positive definite systems at once, each with its own non-pivoting object
 * (as above) or none: ONE launch, one workgroup per system, the whole loop on the device (k_cg_batch, sptrsv_batch.hip).  The layout is
 * that of ilupp_hip_pivot_bicgstab_batch_device, with two differences: members[i] may be NULL (no preconditioner, z = r), and n (a host
 * array of `count`) gives every member's dimension (it must agree with a member's object: ILUPP_ERR_WRONG_SIZE otherwise).  d_work:
 * 5 * sum n_i doubles (x, r, z, p, Ap of every member).  The loop is that of ilupp_amd.device.cg for one column: at most maxiter
 * iterations; every check_every iterations (0: never), when rtol > 0, a member whose ||r|| / ||b|| is at or below rtol stops as
 * converged, before the next apply; a zero right-hand side or initial residual: converged at once, x = x0; p^T A p zero or not finite:
 * the member stops, not converged.  Per member (device arrays of `count`): d_iterations, d_flags (bit 0: still active after maxiter
 * iterations, 1: converged, 2: a sweep gave up -- x untouched, 3: zero right-hand side or initial residual), d_rr = (r, r) at exit and
 * d_bnorm = ||b||.  Every member has the bits of the same solve done alone with ilupp_hip_spmm_device, ilupp_hip_apply_block_device,
 * ilupp_hip_block_dot_device and ilupp_hip_cg_block_update_device.  route (may be NULL): 0 = solved in the launch; 1 = n above the
 * launch's LDS cap (ilupp_hip_cg_batch_max_n); 2 = degenerate factor: members of routes 1 and 2 are NOT solved, their vectors and output
 * words are left untouched.  Ordered on the caller's stream; sync as above.  Refused with ILUPP_ERR_INVALID before any device call: null
 * lists, a negative count, maxiter or check_every, a member named twice, a workspace that is too small, a multilevel handle.
 * count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_cg_batch_device(int32_t count, ilupp_precond *const *members, const int64_t *n, const double *const *d_data,
                              const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz, const double *d_b,
                              const double *d_x0, double *d_x, const int64_t *offsets, double *d_work, int64_t work_doubles, int32_t maxiter,
                              double rtol, int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_bnorm, int sync,
                              int32_t *route);
/* the largest n that takes route 0 in ilupp_hip_cg_batch_device on the current device (ILUPP_BATCH_APPLY_MAX_N applied); negative: an
 * error code */
int64_t ilupp_hip_cg_batch_max_n(void);
/* Left-preconditioned BiCGstab for MANY small systems at once with members of EVERY batched class in the same launch
 * (k_bicgstab_batch, sptrsv_batch.hip): member i's preconditioner is pivoted[i] (an ILUCP / ILUTP object), or plain[i] (ILU0 / ILUT /
 * ILUC / IChol0 / ICholT), or none when both are NULL (r = r0*, Ap = A p, As = A s); either array may be NULL as a whole; both entries
 * non-NULL for one member: ILUPP_ERR_INVALID.  n (a host array of `count`) gives every member's dimension (it must agree with the
 * member's object: ILUPP_ERR_WRONG_SIZE otherwise).  Matrices, vectors, d_work (7 * sum n_i doubles), the loop, the per-member outputs,
 * routes (1 and 2 are NOT solved: the caller solves them one by one), ordering and sync as for ilupp_hip_pivot_bicgstab_batch_device,
 * whose launch this one contains: a pivoting member has the same bits from either entry; a non-pivoting one those of the same solve
 * with ilupp_hip_apply_block_device as its apply.  A re-factorisation (ilupp_hip_ilu0_refactor_device, ..._batch_device) or the
 * destruction of a member is queued behind a launch that was not waited for.  Refused before any device call: null lists, a negative
 * count, maxiter or check_every, n[i] <= 0, a handle named twice within either family, a workspace that is too small, a multilevel
 * handle among `plain`.  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_bicgstab_batch_device(int32_t count, ilupp_precond *const *plain, ilupp_ilucp *const *pivoted, const int64_t *n,
                                    const double *const *d_data, const int32_t *const *d_indices, const int32_t *const *d_indptr,
                                    const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x, const int64_t *offsets,
                                    double *d_work, int64_t work_doubles, int32_t maxiter, double rtol, int32_t check_every,
                                    int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync, int32_t *route);
/* the largest n that takes route 0 in ilupp_hip_bicgstab_batch_device on the current device (ILUPP_BATCH_APPLY_MAX_N applied);
 * negative: an error code */
int64_t ilupp_hip_bicgstab_batch_max_n(void);
/* ilupp_hip_bicgstab_batch_device with a third list: member i is plain[i], pivoted[i], multilevel[i] (each list may be NULL as a whole, at
 * most one of the three non-NULL per member) or a member without a preconditioner.  A launch that holds a multilevel member runs a second
 * instantiation of the kernel (k_bicgstab_batch<true>), in which a member's apply is a choice on its descriptor: a multilevel member walks
 * its levels up and down inside its workgroup as in ilupp_hip_ml_apply_batch_device and has the bits of the same solve done alone with
 * ilupp_hip_ml_apply_device; every other member has the bits it has in ilupp_hip_bicgstab_batch_device.  That instantiation has an LDS cap
 * of its own (ilupp_hip_bicgstab_batch_ml_max_n), by which ALL members of such a launch are routed; where no multilevel member takes
 * route 0 (none given, or all too large or degenerate) the call is ilupp_hip_bicgstab_batch_device's launch with its cap.  Route 2 for a
 * multilevel member: a level object with an empty row.  Everything else -- arguments, outputs, ordering, sync, refusals -- as there; a
 * member of `multilevel` that is not a live multilevel object, or a member named in two lists, is refused with ILUPP_ERR_INVALID. */
int ilupp_hip_bicgstab_batch_ml_device(int32_t count, ilupp_precond *const *plain, ilupp_ilucp *const *pivoted, ilupp_ml *const *multilevel,
                                       const int64_t *n, const double *const *d_data, const int32_t *const *d_indices,
                                       const int32_t *const *d_indptr, const int64_t *nnz, const double *d_b, const double *d_x0, double *d_x,
                                       const int64_t *offsets, double *d_work, int64_t work_doubles, int32_t maxiter, double rtol,
                                       int32_t check_every, int64_t *d_iterations, int32_t *d_flags, double *d_rr, double *d_init, int sync,
                                       int32_t *route);
/* the largest n that takes route 0 in a launch of ilupp_hip_bicgstab_batch_ml_device that holds a multilevel member, on the current
 * device (ILUPP_BATCH_APPLY_MAX_N applied); negative: an error code */
int64_t ilupp_hip_bicgstab_batch_ml_max_n(void);
/* The numeric re-factorisation of MANY small ILU(0) objects at once (same patterns, new values): ONE launch, one workgroup per member,
 * the member's rows side by side inside it (k_ilu0_refactor_batch, ilu0_batch.hip).  members: `count` distinct ILU(0) objects; d_data /
 * d_indices / d_indptr: host arrays of `count` DEVICE pointers, member i's matrix in CSR form as ilupp_hip_ilu0_refactor_device takes
 * it; nnz[i]: its number of stored entries; d_status: a device array of `count` words, member i's being 0 = re-factorised, 1 = the
 * matrix does not have the analysed pattern (proved inside the launch for every row, with no host round trip: the member's factor is
 * bitwise unchanged), 2 = a dependency wait gave up.  Every member's factor has the bits of ilupp_hip_ilu0_refactor_device on the same
 * values, Inf / NaN behind a zero or non-finite pivot included.  route (may be NULL): 0 = the launch; 1 = n above the launch's cap
 * (ilupp_hip_ilu0_refactor_batch_max_n), a longest row above the ROW CAP (a lane's working row lives in LDS: at most 31 entries, and
 * 4 n + 5 120 bytes per entry must fit into a workgroup's LDS -- 28 entries at n = 4 000, 16 at n = 20 000), or a member that would have
 * the launch to itself and has 1 000 rows or more (alone it is faster on the single path); 2 = static form (the values live in
 * lane-table records): members of
 * routes 1 and 2 are re-factorised by ilupp_hip_ilu0_refactor_device's path inside the call (with its host waits), their status words
 * written afterwards.  Ordered on the caller's stream; the launch comes after whatever is queued on a member's own stream, and the
 * member's own stream (single applies, ilupp_hip_factor_copy) and every later batched launch come after it.  sync == 0: nothing is
 * waited for, unless a launched member still holds copies of the old values that have to be freed (packed, transposed or level-ordered
 * sweeps of single applies: one wait for the whole call; members used through ilupp_hip_cg_batch_device / the plain
 * ilupp_hip_apply_batch_device hold none).  sync != 0: the call waits and returns ILUPP_ERR_INVALID / ILUPP_ERR_TIMEOUT naming the first
 * member whose status is 1 / 2.  Refused with ILUPP_ERR_INVALID before any device call: null lists or members, a negative count, a
 * member named twice, a multilevel handle, a member that is not an ILU(0) object, nnz[i] that is not the analysed pattern's ("member i
 * of the batch: the matrix does not have the analysed pattern").  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_ilu0_refactor_batch_device(int32_t count, ilupp_precond *const *members, const double *const *d_data,
                                         const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz,
                                         int32_t *d_status, int sync, int32_t *route);
/* the largest n that takes route 0 in ilupp_hip_ilu0_refactor_batch_device on the current device (ILUPP_BATCH_APPLY_MAX_N applied);
 * negative: an error code */
int64_t ilupp_hip_ilu0_refactor_batch_max_n(void);
/* The FIRST construction of MANY small ILU(0) objects at once: a symbolic launch and a create launch of one workgroup per member
 * (k_ilu0_symbolic_batch, k_ilu0_create_batch: ilu0_batch.hip) around ONE read-back, where a loop of ilupp_hip_ilu0_create* pays the single
 * path's analysis and host waits per object.  ilupp_hip_ilu0_create_batch takes host CSR arrays (all members are staged through one packed
 * block with one upload), ilupp_hip_ilu0_create_batch_device host arrays of `count` DEVICE pointers, n[i] and nnz[i] (member i's number
 * of stored entries; a member whose indptr[n] differs is refused).  is_csr as for ilupp_hip_ilu0_create (CSC input: the row-major view
 * is factored).  out: `count` handles (ilupp_hip_destroy); status (may be NULL): member i's code; route (may be NULL): 0 = built by the
 * launches, 1 = built by ilupp_hip_ilu0_create* inside the same call -- n above ilupp_hip_ilu0_refactor_batch_max_n(), a longest row
 * above the row cap of ilupp_hip_ilu0_refactor_batch_device, a matrix with an unsorted row or an index out of range (whatever the single
 * constructor does with it happens here), or a batch of ONE member (who builds one object wants the fully analysed one).
 * A route-0 object holds L and U as CSR triangles with their values and none of the single paths' analysis: factors, total_nnz and every
 * apply have the bits of ilupp_hip_ilu0_create's object, ilupp_hip_path is "ilu0:batch", the batched launches (ilupp_hip_apply_batch_device,
 * ilupp_hip_cg_batch_device, ilupp_hip_bicgstab_batch_device, ilupp_hip_ilu0_refactor_batch_device: always route 0 there) take it as it is,
 * the tables of the single sweeps are built at its first single apply, ilupp_hip_ilu0_refactor_device runs the batched launch with that one
 * member, and ilupp_hip_get_timings reports the two launches' times (analysis_ms, numeric_ms), shared by the call's members.
 * The launches run on the library's batch stream behind the caller's (ilupp_hip_set_caller_stream); the call returns when every member is
 * built.  A member that fails fails as its single construction does ("matrix i of the batch: ILU0: structurally missing diagonal entry in
 * row r"): the first failure is returned, status[i] says which members failed, every object of the call is destroyed and no handle is
 * returned.  count == 0 returns ILUPP_OK without touching the device. */
int ilupp_hip_ilu0_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                const int32_t *n, int is_csr, ilupp_precond **out, int32_t *status, int32_t *route);
int ilupp_hip_ilu0_create_batch_device(int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                                       const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, ilupp_precond **out,
                                       int32_t *status, int32_t *route);

/* IChol(0) for MANY small SPD systems: what the five entries above are for ILU(0) (k_ichol0_refactor_batch, k_ichol0_symbolic_batch,
 * k_ichol0_create_batch: ichol0_batch.hip; one workgroup per member, one lane per row).
 * ilupp_hip_ichol0_refactor_device is the single numeric re-factorisation (same pattern, new values): the matrix's stored entries with
 * column <= row must be, row by row and in stored order, the rows of the factor (entries above the diagonal are ignored, as the
 * constructor drops them); a matrix that differs returns ILUPP_ERR_INVALID ("IChol0 refactor: the matrix does not have the analysed
 * pattern") and leaves the factor bitwise unchanged.  The factor has the bits of ilupp_hip_ichol0_create on the same values; every copy
 * of the old values (transposed storage, packed and level-ordered sweeps) goes and is rebuilt on first use.  A batch-built object runs
 * the batched launch with that one member.
 * ilupp_hip_ichol0_refactor_batch_device: arguments, ordering, sync, status words and refusals as for
 * ilupp_hip_ilu0_refactor_batch_device ("not an IChol(0) object" for other members; nnz[i] is the matrix's number of stored entries,
 * upper triangle included).  route: 0 = the launch; 1 = n above ilupp_hip_ichol0_refactor_batch_max_n(), a longest row of L above the
 * row cap (at most 31 entries, and 4 n + 5 120 bytes per entry must fit into a workgroup's LDS: 28 entries at n = 4 000, 16 at
 * n = 20 000), or a member that would have the launch to itself and has ILUPP_REFACTOR_ALONE_MIN rows or more; 2 = an object whose
 * constructor ran the static form: routes 1 and 2 take ilupp_hip_ichol0_refactor_device's path inside the call.  The launch also writes
 * the new values into a member's transposed storage when it has one (ilupp_hip_cg_batch_device and ilupp_hip_apply_batch_device read the
 * factor and that copy): a route-0 member keeps both, and a steady state of re-factorisation -> ilupp_hip_cg_batch_device ->
 * re-factorisation waits for nothing on the host and launches nothing per member.  With status 1 the factor and the transposed copy
 * are bitwise as they were.
 * ilupp_hip_ichol0_create_batch / _device: as ilupp_hip_ilu0_create_batch / _device (is_csr is ignored, as in ilupp_hip_ichol0_create).
 * A route-0 object has the bits of ilupp_hip_ichol0_create's, ilupp_hip_path is "ichol0:batch"; a failing member fails as its single
 * construction does ("matrix i of the batch: IChol0: structurally missing diagonal entry in row r"). */
int ilupp_hip_ichol0_refactor_device(ilupp_precond *p, const double *d_data, const int32_t *d_indices, const int32_t *d_indptr);
int ilupp_hip_ichol0_refactor_batch_device(int32_t count, ilupp_precond *const *members, const double *const *d_data,
                                           const int32_t *const *d_indices, const int32_t *const *d_indptr, const int64_t *nnz,
                                           int32_t *d_status, int sync, int32_t *route);
int64_t ilupp_hip_ichol0_refactor_batch_max_n(void);
int ilupp_hip_ichol0_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                  const int32_t *n, int is_csr, ilupp_precond **out, int32_t *status, int32_t *route);
int ilupp_hip_ichol0_create_batch_device(int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                                         const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, ilupp_precond **out,
                                         int32_t *status, int32_t *route);

/* The FIRST construction of MANY small ILUT(max_fill_in, threshold) objects at once (one parameter set per batch).  ILUT's pattern depends
 * on the values, so there is no numeric re-factorisation to fall back on: a time-stepping caller builds every member again at every step,
 * and a loop of ilupp_hip_ilut_create* pays per member the record initialisation, the rows kernel running nearly empty, five host waits
 * and the waves' working arrays.  Here all members share k_ilut_rows_batch (ilut_wp.hip): the single kernel's wave loop -- the same
 * wp_row, the same three capacity tiers, the same bits -- over the rows of ALL members, claimed round-robin (round r holds row r of
 * every member that has one: within a member rows are claimed in ascending order, so a row still waits only on rows claimed earlier, and
 * the members' dependency chains run side by side), then one count-and-scan launch, ONE read-back (per member: status, first row with a
 * zero pivot, nnz(L), nnz(U), longest row) and one fill launch that drops exact zeros as the single path's compaction does.
 * Arguments as for ilupp_hip_ilu0_create_batch / _device, plus max_fill_in and threshold as for ilupp_hip_ilut_create.  route (may be
 * NULL): 0 = built by the launches; 1 = built by ilupp_hip_ilut_create* inside the same call -- a batch of ONE member, a clamped budget
 * min(max(max_fill_in, 1), n) - 1 >= 256 (the largest capacity class, which the launch does not have), or a member whose launch met a row
 * that fits no tier of it.  A route-0 object holds L and U with their values, the longest row of the two, and nothing else: factors,
 * total_nnz and every apply have the bits of ilupp_hip_ilut_create's object, ilupp_hip_path is "ilut:batch", the batched launches take it
 * as it is, the tables of the single sweeps are built at its first single apply, and ilupp_hip_get_timings reports the rows launches as
 * numeric_ms, shared by the call's members.  The re-factorisation entries refuse it as they refuse every ILUT object.
 * A member with a zero pivot fails as its single construction does ("matrix i of the batch: ILUT_heap: encountered zero pivot in row N"), a
 * dependency wait that timed out is ILUPP_ERR_TIMEOUT: the first failure is returned, status[i] says which members failed, every object
 * of the call is destroyed and no handle is returned.  count == 0 returns ILUPP_OK without touching the device; null arguments are
 * refused before any HIP call ("null argument"). */
int ilupp_hip_ilut_create_batch(int32_t count, const double *const *data, const int32_t *const *indices, const int32_t *const *indptr,
                                const int32_t *n, int is_csr, int32_t max_fill_in, double threshold, ilupp_precond **out, int32_t *status,
                                int32_t *route);
int ilupp_hip_ilut_create_batch_device(int32_t count, const double *const *d_data, const int32_t *const *d_indices,
                                       const int32_t *const *d_indptr, const int32_t *n, const int64_t *nnz, int is_csr, int32_t max_fill_in,
                                       double threshold, ilupp_precond **out, int32_t *status, int32_t *route);

/* ---------------------------------------------------------------------------------------------
 * Measurement hooks used by bench.py (not part of the reference's surface).
 * Times are GPU milliseconds from hipEvents recorded on the object's stream.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float analysis_ms;   /* symbolic pass: diagonal positions, L/U pattern split, row scheduling */
    float numeric_ms;    /* numeric factorisation kernel(s) */
    float last_apply_ms; /* most recent apply / apply_trans on device data */
    float numeric_kernel_ms;  /* the dominant numeric kernel alone */
    float lsolve_kernel_ms;   /* forward-solve kernel of the last apply */
    float usolve_kernel_ms;   /* backward-solve kernel of the last apply */
} ilupp_timings;
int ilupp_hip_get_timings(const ilupp_precond *p, ilupp_timings *t);
/* which kernel family built this object ("ilu0:static-direct", "ilu0:static-level-major", "ilu0:level-order",
 * "ilu0:csr-program", "ilu0:csr", "ilu0:batch", "ilut", "ilut:batch", "ichol0", "ichol0:batch", "icholt"): bench.py names the kernel its roofline line is about */
const char *ilupp_hip_path(const ilupp_precond *p);
/* how the row blocks of an ILU(0) object were found: "grid" (the pattern is a lexicographic box-grid stencil: guessed from row 0, proven
 * for every row by one streaming pass next to the lane-table kernels, grid.hip) or "general" (the pass over the pattern that finds the
 * chains of any matrix, symbolic.hip); "" for other objects.  Measurement / test hook, no counterpart in binding.cpp. */
const char *ilupp_hip_analysis_path(const ilupp_precond *p);
/* diagnostics (tests compare the closed-form tables of grid.hip with the ones the general kernels make): table `which` of a static ILU(0)
 * object as 32-bit words -- 0 / 1 lane tables (forward / backward schedule), 2 / 3 chunk tables, 4 backward right-hand-side map, 5 rows-pass
 * records, 6 / 7 export ordinals, 8 / 9 exchange layout, 10 forward -> backward slots, 11 / 12 skews; returns the words copied (<= cap), -1
 * where there is no such table.  No counterpart in binding.cpp. */
long long ilupp_hip_debug_static_table(ilupp_precond *p, int which, int32_t *out, long long cap);
/* diagnostics (tests compare the level numbering with a CPU model and pin the kernel family of every sweep): the level order of slot `which`
 * as perm[position] = row -- 0 .. 3 the level-ordered copies of L, U, U^T, L^T as stored (the slots of an apply's two sweeps), 4 the factor
 * order of an "ilu0:level-order" object.  info[0] levels, [1] / [2] window and block size of the sweep kernel, [3] how the order was numbered
 * (0 given: a copy of the factor order, 1 natural-order pass, 2 relaxation converged, 3 relaxation given up, then the natural-order pass),
 * [4] batches of relaxation passes run, [5] window of the natural-order pass (0: none ran), [6] kernel family of the LAST sweep over the slot
 * (0 none yet, 1 static, 2 level-major, 3 level order, 4 one lane per row in natural order, 5 the same because a factor is degenerate,
 * 6 descriptor kernels, 7 generic kernel; 0 for which = 4), [7] the kernel inside family 6 (1 k_sptrsv_lc, 2 k_sptrsv_desc; 0 for every other
 * family).  Builds nothing (call an apply first) and waits for the object's stream.
 * Returns the words copied (<= cap), -1 where that order does not exist (never tried, declined, dropped by a re-factorisation); info[6] and
 * info[7] are valid either way.  No counterpart in binding.cpp. */
long long ilupp_hip_debug_level_order(ilupp_precond *p, int which, int32_t *perm_out, long long cap, int32_t info[8]);
/* measurement hook: the kernels a static ILU(0) object runs, "factor;forward sweep;backward sweep"; for an LL^T object (IChol0, ICholT) its
 * factor kernel and, once an apply has built them, the sweeps of its factor pair; "" otherwise.  No counterpart in binding.cpp */
const char *ilupp_hip_kernel_names(const ilupp_precond *p);
/* redo the numeric phase on (possibly new) values with the SAME pattern (buffers reused); times it */
int ilupp_hip_ilu0_refactor_device(ilupp_precond *p, const double *d_data, const int32_t *d_indices,
                                   const int32_t *d_indptr);
/* wait for asynchronous applies (ilupp_hip_apply_device with sync=0) and report their status */
int ilupp_hip_sync(ilupp_precond *p);
/* The library keeps freed device buffers (up to a limit, the oldest go first) for the next construction: a factorisation that is
 * repeated asks for the same sizes again and hipMalloc / hipFree of multi-GB buffers cost more than the kernels.  This hands them
 * back to the driver (no counterpart in binding.cpp: the reference's buffers are host memory).
 * The cache also holds PARKED PLANS: when an ILU(0) object of a box-grid matrix is destroyed, the tables its analysis made from the grid's
 * dimensions alone (schedules, lane tables: tens of MB at 256^3, none of the value records) are kept for the next ILU(0) object of the
 * same device, size, entry count and dimensions, which then skips that part of the analysis (the proof of the pattern still runs every
 * time).  A few plans per device, the least recently parked leaves first; only objects that saw nothing but their construction and
 * plain, waited-for applies leave one.  ILUPP_NO_PLAN_CACHE=1 turns it off.  This call drops every parked plan as well. */
int ilupp_hip_release_cached_memory(void);
/* the limit of that cache in bytes (default 48 GiB, or ILUPP_CACHE_LIMIT_MB; 0 = keep nothing); blocks over the new limit are
 * handed back at once.  A process that shares the GPU with other allocators sets this before its first factorisation.
 * Parked plans count against the limit: one that would exceed it is not parked, and a lower limit drops plans first. */
int ilupp_hip_set_cache_limit(unsigned long long bytes);
/* bytes currently kept in the cache, parked plans included / blocks currently handed out, parked plans' blocks NOT included
 * (diagnostics; a leak shows as blocks that never come back) */
unsigned long long ilupp_hip_cached_bytes(void);
unsigned long long ilupp_hip_live_blocks(void);
/* diagnostics of the parked plans: out[0] = plans parked now, out[1] = constructions that adopted one, out[2] = constructions of a
 * box-grid shape that found none, out[3] = plans that left unused (evicted, released with the cache, over the limit, or adopted for a
 * matrix that then failed the proof).  No counterpart in binding.cpp. */
int ilupp_hip_plan_cache_stats(unsigned long long out[4]);

#ifdef __cplusplus
}
#endif
#endif
