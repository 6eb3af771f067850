// Internal declarations shared by the HIP translation units of
// libraoteh_hip.so.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/raoteh_hip.h"

// ---- error plumbing ---------------------------------------------------------

void rt_set_error(const char *fmt, ...);

#define RT_HIP(call)                                                          \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            rt_set_error("%s failed: %s (%s:%d)", #call,                      \
                         hipGetErrorString(e_), __FILE__, __LINE__);          \
            return RT_ERR_HIP;                                                \
        }                                                                     \
    } while (0)

#define RT_REQUIRE(cond, ...)                                                 \
    do {                                                                      \
        if (!(cond)) {                                                        \
            rt_set_error(__VA_ARGS__);                                        \
            return RT_ERR_INVALID;                                            \
        }                                                                     \
    } while (0)

#define RT_TRY(...)                                                           \
    do {                                                                      \
        int rc_ = (__VA_ARGS__);                                              \
        if (rc_ != RT_OK) return rc_;                                         \
    } while (0)

// ---- what the host side of the calls shares ----------------------------------

// device allocations freed when the guard goes, but those released to a longer-lived owner
struct dev_free {
    std::vector<void *> ptrs;
    ~dev_free() { for (void *p : ptrs) hipFree(p); }
    template <class T> int alloc(T *&p, size_t count)
    {
        p = nullptr;
        RT_HIP(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
        ptrs.push_back(p);
        return RT_OK;
    }
    template <class T> T *release(T *p)
    {
        for (void *&q : ptrs) if (q == p) q = nullptr;
        return p;
    }
};

// A call's pieces of the context's grow-only device scratch: byte offsets, 256-byte aligned,
// bumped out of one plan; rt_scratch_reserve(ctx, plan.total) then makes ctx->d_scratch hold them
// all (valid until the next reserve)
struct post_plan {
    size_t total = 0;
    size_t take(size_t bytes)
    {
        const size_t o = total;
        total += (bytes + 255) / 256 * 256;
        return o;
    }
};
// f(std::integral_constant<int, V>) for the V in LO .. HI that equals v, RT_ERR_UNSUPPORTED for
// any other v: the one table of the kernels' template arguments.  The lane kernels take the
// states, the wave-per-tile kernels the row tiles NT (1 .. 8), the downward kernels the k-steps
// KS (2 .. 32) with NT = ceil(KS / 4).
template <int LO, int HI, class F>
inline int post_dispatch(int v, F &&f)
{
    if constexpr (LO > HI) return RT_ERR_UNSUPPORTED;
    else return v == LO ? f(std::integral_constant<int, LO>()) : post_dispatch<LO + 1, HI>(v, f);
}

struct rt_jit_job;      // a background compile (jit.hip)

// ---- handles ------------------------------------------------------------------

struct rt_timing_slot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<hipEvent_t> pool;
    double total_ms = 0.0;
    int64_t launches = 0;
    int64_t seen = 0;
    char name[64] = "";        // variant that ran last (owned by the slot: no statics)
};

static const int RT_TOTALS_SLOTS = 4096;   // site batches per context sharing the arena

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 0;
    bool timing = false;
    int timing_period = 1;
    rt_timing_slot slots[RT_K_COUNT];
    // events of the launch being timed (rt_time_begin .. rt_time_end), else null
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // totals of every site batch of this context live in one arena ([slot][3] doubles)
    // so that the totals of several batches can be all-reduced by ONE collective
    double *d_totals_arena = nullptr;
    std::vector<int> totals_free;          // free slots, highest index last popped first
    hipEvent_t ev_reduced = nullptr;       // compute stream: totals of a group written
    hipEvent_t comm_events[8] = {};        // comm stream: a collective finished (ring)
    int comm_event_next = 0;
    // grow-only device scratch of the reference-format calls (no hipMalloc / hipFree
    // per call: single-site calls are latency-bound)
    unsigned char *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    void *comm = nullptr;          // ncclComm_t
    hipStream_t comm_stream = nullptr;   // collectives overlap the next step's kernels
    void *rccl = nullptr;          // dlopen handle
    // options snapshotted by rt_sites_create (rt_ctx_set_option); RT_OPT_UNSET = the
    // process-wide default of rt_set_option applies
    int opt_force_generic = -2;
    int opt_jit = -2;
    int opt_jit_block_sites = -2;
    int opt_jit_async = -2;
    int opt_rescale = -2;
    int opt_leaf_state_kernels = -2;
    // The batch whose per-wave partial sums still await their fixed-order reduction.
    // rt_step defers it: the reduction of step j rides as one extra workgroup of step
    // j + 1's expm launch (two launches per step instead of three: on config 2 the two
    // launch-latency-sized kernels were a quarter of the step); every reader of the
    // totals, rt_prune, rt_ctx_sync and the destructors flush it (rt_flush_reduce).
    struct rt_sites *pending_reduce = nullptr;
    // The root-halves batch whose combine has not run yet: rt_step leaves it to the next expm
    // launch of this context, whose waves 4..7 idle until the first barrier (expm.hip).  Its
    // per-site results and partial sums exist after that launch, so its reduction rides one
    // launch later still.  rt_flush_pending runs both now.
    struct rt_sites *pending_combine = nullptr;
    size_t expm_attr_lds = 0;      // dynamic-LDS attribute already granted to expm_kernel
    size_t expm_ts_attr_lds[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ... to the Taylor kernels (per NT)
    size_t expm_split_attr_lds = 0;                           // ... to the two-workgroup form
    size_t expm_w8_attr_lds[3] = {0, 0, 0};    // ... to the eight-wave forms: NT = 3, 4, pair
    size_t expm_wide_attr_lds[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double *d_expm_scratch = nullptr;   // matrices of the order > 64 Taylor kernel (grow-only)
    void *expect_cache = nullptr;       // expect_mfma.hip: model + packed batch of the last call
    size_t expm_scratch_bytes = 0;
    // Lifetime (include/raoteh_hip.h, "ownership and destruction order"): a context cannot
    // go while one of its models or chain batches lives, a model not while one of its site
    // batches lives -- the destroy call refuses (RT_ERR_INVALID) instead of leaving the
    // children with a dangling parent.  Counts of live children, own internal objects (the
    // expectation cache, probe batches) included.
    int live_models = 0, live_chains = 0;
};
static const int RT_OPT_UNSET = -2;

// One schedule step of the fast pruning kernels: a node of the tree visited in
// post-order.  For a non-root node v the step forms L_v (pop its accumulator if
// internal, multiply its observation in), t = P_v * L_v and folds t into its
// parent's accumulator slot; the final step (dst = -1) is the root reduction.
static const int RT_FAST_MAX_DEPTH = 16;   // LDS accumulator stack of the fast kernels

struct rt_op {
    int32_t node;      // preorder index of v (also the P slot of edge parent->v)
    int32_t obs;       // position of v in the observation stream, or -1
    int32_t pop;       // accumulator slot of v (internal node), or -1 (leaf)
    int32_t dst;       // parent's accumulator slot | (first child ? 256 : 0); -1 root
};

// rt_model_set_rate_sets: K rate sets next to the state rt_model_set_rates owns.  Every table a
// pruning kernel reads exists K times, set k at k * (its per-set stride): one expm launch over
// K * nnodes matrices fills them all (the rate-matrix index and the step index of an edge are
// offset by its set, so the epilogue's step-ordered stores land in the set's own tables).
struct rt_rate_sets {
    int64_t K = 0;                  // sets resident (0: rt_model_set_rate_sets not called yet)
    int64_t capacity = 0;           // sets the tables are allocated for (grow-only)
    int64_t nq = 0, q_capacity = 0; // rate matrices per set / K * nq the buffer holds
    uint64_t epoch = 0;             // bumped whenever K changes: results of another K are stale
    double *d_Q = nullptr;          // [K][nq][n][n]
    int32_t *d_qidx = nullptr;      // [K][nnodes], set k's entries + k * nq (root: -1)
    double *d_t = nullptr;          // [K][nnodes]
    std::vector<int32_t> h_node_q;  // [nnodes] the rate matrix of every node within a set, shared by
                                    // the sets (root: -1); the host's copy of what d_qidx holds
    int32_t *d_info = nullptr;      // [K][nnodes][2]
    int32_t *d_step_of_node = nullptr;  // [K][nnodes], set k's entries + k * steps per set
    double *d_P = nullptr;          // [K][nnodes][n][n]
    double *d_Pfrag = nullptr, *d_Pquad = nullptr, *d_Pcol = nullptr;
    int64_t pcol_capacity = 0;
    int64_t P_stride = 0, frag_stride = 0, quad_stride = 0, pcol_stride = 0;   // doubles per set
};

struct rt_model {
    rt_ctx *ctx = nullptr;
    int64_t nnodes = 0;
    int64_t n = 0;
    std::vector<int64_t> indices, indptr;   // host copy of the CSR
    std::vector<int32_t> parent;            // preorder parent index, -1 root
    std::vector<rt_op> ops;                 // post-order schedule
    std::vector<int32_t> h_qidx;            // what d_qidx / d_t hold (rt_model_set_rates)
    std::vector<double> h_t;
    int max_depth = 0;                      // accumulator slots needed
    // device
    int64_t *d_indices = nullptr, *d_indptr = nullptr;
    rt_op *d_ops = nullptr;
    double *d_P = nullptr;          // [nnodes][n][n] esd_transitions
    double *d_Pfrag = nullptr;      // MFMA A-fragment order (n > 4)
    // 4 < n <= 32: the same matrices as 4 x 4 blocks [step][row quad][col quad][k][i] =
    // P[4 rq + i][4 kk + k], what the v_mfma_f64_4x4x4_4b kernels of jit.hip read (the
    // four blocks of that instruction share A: 4 rows x 16 sites per instruction, so 20
    // states cost 5 x 5 instructions of 16 cycles instead of 2 x 5 of 64)
    double *d_Pquad = nullptr;
    // leaf-column table for the split-M leaf-state kernels (jit.hip, `sparse`): column s of the
    // step's P with the four rows a lane owns adjacent, Pcol[rec][s][m][lane >> 4][r] =
    // P[16 m + 4 r + (lane >> 4)][s]; allocated when the first such batch is created, rewritten
    // whenever the transition matrices change
    double *d_Pcol = nullptr;
    double *d_root = nullptr;       // [n] root weights (ones if unset)
    // rt_model_set_rates_spectral: A [n][n], B [n][n], lam [n], D [n] of the decomposition
    // (spectral.hip); while `spectral` is set the transitions are rebuilt from these
    double *d_spec = nullptr;
    bool spectral = false, spectral_has_D = false;
    double *d_Q = nullptr;          // rate matrices of the last set_rates
    int64_t q_capacity = 0;
    int32_t *d_qidx = nullptr;      // [nnodes]
    double *d_t = nullptr;          // [nnodes]
    int32_t *d_info = nullptr;      // [nnodes][2]
    int32_t *d_step_of_node = nullptr;  // [nnodes] schedule step of each node
    // the same rate-matrix indices / branch lengths in STEP order (the root's step: -1, 0): a
    // lane kernel that computes its own transitions reads them at its thread index, with no
    // step -> node lookup in front of the loads (n <= 4 only)
    int32_t *d_qidx_step = nullptr;
    double *d_t_step = nullptr;
    bool have_P = false;
    // the transition matrices are those of the resident rates (rt_model_set_rates / _spectral,
    // a recompute); rt_model_set_transitions clears it: the rates no longer describe P
    bool rates_current = false;
    bool frag_dirty = true;
    int live_batches = 0;           // site batches created from this model and not yet destroyed
    void *expect_state = nullptr;   // expect_mfma.hip: device buffers of rt_expect_step (lazy)
    void *expect_lane_state = nullptr;  // passes.hip: its n <= 8 form (plan, pattern bits)
    rt_rate_sets multi;             // rt_model_set_rate_sets (buffers allocated on first use)
};

// Device layouts of a site batch:
//  RT_LAYOUT_LANE  (n <= 4)  [block of 64 sites][obs slot][lane][np] f64,
//                  np = n rounded up to even: one lane owns one site
//  RT_LAYOUT_MFMA  (n  > 4)  [block of 16 sites][obs slot][k-step pair][lane][2]
//                  f64 in v_mfma_f64_16x16x4 B-operand order
enum { RT_LAYOUT_LANE = 0, RT_LAYOUT_MFMA = 1 };

// rt_sites_create_partitioned: site i under rate set site_set[i].  The batch is resident in the
// planner's order (partition_plan.h): s->nsites counts its SLOTS (pads included), every granule of
// G slots belongs to one set, and the pruning launch looks the set up per granule.  The caller's
// order exists in the gathered copies and in the per-set reductions only.
struct rt_partition {
    int64_t nsites = 0;             // the caller's sites
    int64_t nsets = 0, G = 0, padded = 0;
    int64_t *d_order = nullptr;         // [padded] source site of every slot
    int64_t *d_slot_of_site = nullptr;  // [nsites]
    uint8_t *d_is_pad = nullptr;        // [padded]
    int32_t *d_granule_set = nullptr;   // [granules the kernel's grid covers]
    int64_t *d_run_begin = nullptr;     // [nsets + 1]
    std::vector<int64_t> run_begin;     // (its host copy: an empty run is a set without a site)
    double *d_loglik = nullptr;         // [nsites] caller order (gathered after every step)
    int32_t *d_status = nullptr;
    int nblocks = 1;                    // stage-1 workgroups per set (from the plan alone)
    double *d_totals = nullptr;         // [nsets][3], [nsets] weighted sums, [nsets][nblocks][4]
    bool stepped = false;               // an rt_step_partitioned has written the results
    uint64_t epoch = 0;                 // the model's rate-set epoch and K at that step
    int64_t model_K = 0;
    int64_t device_bytes = 0;           // of the arrays above (rt_sites_device_bytes adds them)
};

struct rt_sites {
    rt_model *model = nullptr;
    int64_t nsites = 0;
    int64_t nobs = 0;
    int layout = RT_LAYOUT_LANE;
    bool lane_dma = false;          // lane family: LDS-DMA ring instead of VGPR ring
    int lane_ring = 8;              // ring depth of the lane kernel
    bool mfma_solo = false;         // MFMA family, n <= 32: one wave owns a tile outright
    int64_t nblocks = 0;            // site blocks (64 or 16 sites each)
    int64_t obs_bytes = 0;
    std::vector<int32_t> node_obs;  // per node: stream position or -1
    std::vector<rt_op> ops;         // model ops with .obs filled in
    rt_op *d_ops = nullptr;
    int32_t *d_lane_ops = nullptr;  // lane-kernel program (int32[nprog][4])
    int lane_stack_slots = 1;       // LDS accumulator slots the program touches
    int64_t lane_nprog = 0;         // its entries (< steps when cherries are fused)
    double *d_obs = nullptr;
    double *d_loglik = nullptr;     // [nblocks * sites per block]
    int32_t *d_status = nullptr;
    double *d_partial = nullptr;    // [npartials][2] (sum, nzero)
    int64_t npartials = 0;
    double *d_totals = nullptr;     // [3]: a slot of the context's arena (or its own)
    int totals_slot = -1;           // arena slot, -1: d_totals is its own allocation
    hipEvent_t ev_comm_done = nullptr;  // ctx-owned: the collective that last touched the totals
    bool comm_pending = false;
    void *jit_fn = nullptr;         // hipFunction_t of the tree-specialised kernel (jit.hip)
    int jit_prefetch = 0;           // its prefetch distance (stream positions)
    int jit_lookahead = 1;          // ... and P records requested ahead
    int block_sites = 64;           // lane family: sites per block (< 64 only with jit_fn)
    int jit_waves = 1;              // waves per workgroup of the tree-specialised kernel
    int jit_tiles = 1;              // MFMA family: site tiles per wave of that kernel
    bool jit_quad = false;          // ... built on v_mfma_f64_4x4x4_4b (reads d_Pquad)
    // split-M family, root halves (jit.hip): the two root programs run as the even / odd
    // workgroups of jit_fn and leave their share of the root's accumulator in d_half
    // ([tile][half][k-step][lane]); jit_combine (same module) finishes the sites
    // lane family: the kernel can compute the transition matrices of a step in its own
    // prologue (jit.hip, `fuse`); rt_step then launches ONE kernel.  The batch sum of step j
    // rides as an extra workgroup of step j + 1's launch while that launch writes its own
    // partial sums: two buffers, swapped at every such launch
    bool jit_fused = false;
    double *d_partial_alt = nullptr;
    bool jit_halves = false;
    void *jit_combine = nullptr;
    double *d_half = nullptr;
    // folded form: the second workgroup of a pair to arrive finishes the pair's tiles (no
    // combine launch); d_half_count: one arrival counter per pair, zero between launches
    bool jit_fold = false;
    bool jit_teams = false;         // ... two four-wave teams per workgroup (jit.hip)
    int *d_half_count = nullptr;
    // the same cut for the split-M INTERPRETER kernel (prune.hip rt_interp_halves), used while
    // the batch has no tree-specialised kernel: the two root programs, the P record and the
    // stream position the second one starts at, the root's own stream position (-1: none)
    bool interp_halves = false;
    // "rescale" option at creation: messages rescaled by powers of two, exponent per site
    // (interpreter kernels only; such a batch never gets a tree-specialised kernel)
    bool rescale = false;
    int32_t *d_lane_ops_a = nullptr, *d_lane_ops_b = nullptr;
    // expectation path (expect_mfma.hip): per step {slot of the parent's D, own slot or -1}
    int32_t *d_down_meta = nullptr;
    int down_slots = 0;
    int half_nops[2] = {0, 0};
    int half_rec1 = 0, half_kobs1 = 0, half_kroot = -1;
    // not owned: where the split-M interpreter kernel leaves L_v and M_v of every step
    // (expect_mfma.hip sets them around its own launch)
    double *d_Lout = nullptr, *d_Mout = nullptr;
    int compact_states = 0;         // lane family + specialised kernel: the batch stays resident
                                    // as one byte per leaf: 1 = uint8 states, 2 = allowed-set masks
    double *d_scratch = nullptr;    // generic kernel message stack
    int64_t scratch_bytes = 0;
    // background compile of the tree-specialised kernel (MFMA family): the batch runs the
    // interpreter kernel until the job is done and rt_sites_jit_poll swaps the kernel in
    std::shared_ptr<rt_jit_job> jit_job;
    struct jit_cand { int T; bool halves; bool quad; bool sparse = false; bool pipe = false;
                      bool teams = false; };
    std::vector<jit_cand> jit_cands;        // what each candidate source of the job was built with
    std::vector<std::string> jit_srcs;
    int jit_kind = 0;                       // observation kind of the batch (probe batches)
    // lane family (n <= 4): the kernel's resident layout differs from the interpreter's, so
    // while the job runs the batch keeps the caller's observations on the device (d_raw, in
    // the caller's format) and packs them again at the switch; what the kernel was built for:
    bool keep_raw = false;
    void *d_raw = nullptr;
    int *d_raw_src = nullptr;
    struct { int S = 64, WG = 1, D = 1, LA = 1, compact = 0; bool fuse = false; } jit_lane;
    // n > 32, observed STATES at leaves only, none unobserved: next to the dense image the
    // batch keeps the state bytes (leafw[tile][ceil(K/4)][16 sites], four stream positions per
    // word) for the tree-specialised kernel whose leaf steps gather columns of P (jit.hip)
    bool sparse_ok = false;
    bool sparse_pairs = false;       // ... as allowed sets of one or two states (RT_OBS_MASK): 16 bits per leaf
    bool jit_sparse = false;
    bool jit_pipe = false;                  // ... from the pipelined generator (leaves as factors)
    unsigned *d_leafw = nullptr;
    // rt_expect_step: per-site multiplicities on the device (null: ones), and the batch's
    // split-M interpreter twin -- its own program, partial sums and per-site outputs over the
    // SAME resident observations (obs_borrowed: d_obs belongs to the batch it was made from)
    double *d_weights = nullptr;
    unsigned char *d_sets = nullptr;        // n <= 8: allowed sets [node][site] (built once)
    rt_sites *expect_twin = nullptr;
    bool obs_borrowed = false;
    bool counted = false;           // this batch is in its model's live_batches
    // a pruning launch has written d_loglik / d_status (or a clone copied them): before that
    // they hold nothing and rt_sites_get_logliks refuses
    bool pruned = false;
    char kernel_name[64] = "";      // the pruning kernel variant of this batch
    // rt_step_multi: per-set results [K][...] next to the batch's own (allocated on first use,
    // again when K grows or the batch changes its resident layout)
    int64_t multi_capacity = 0;     // sets the buffers hold
    int64_t multi_padded = 0, multi_npartials = 0;   // per-set strides they were allocated with
    int64_t multi_K = 0;            // sets of the last rt_step_multi (0: none yet)
    uint64_t multi_epoch = 0;       // the model's rate-set epoch at that step
    void *multi_last_fn = nullptr;  // kernel that last wrote d_mpartial (another one: zero them)
    bool multi_last_valid = false;
    double *d_mloglik = nullptr;    // [K][multi_padded]
    int32_t *d_mstatus = nullptr;   // [K][multi_padded]
    double *d_mpartial = nullptr;   // [K][multi_npartials][2]
    double *d_mtotals = nullptr;    // [K][3], then [K] weighted sums
    char multi_kernel_name[80] = "";
    // one launch for all sets (split-M family, 33..64 states): the batch's own kernel form
    // generated with the multi prologue (jit.hip), a cache entry of its own.  multi_state:
    // 0 not asked for yet, 1 compiling in the background, 2 verified and in use, -1 none
    // (rejected or failed: the loop form runs); multi_for: the batch kernel it belongs to
    int multi_state = 0;
    void *multi_fn = nullptr, *multi_combine = nullptr, *multi_for = nullptr;
    std::shared_ptr<rt_jit_job> multi_job;
    std::string multi_src;
    double *d_mhalf = nullptr;      // [K][multi_half_stride] root halves per set
    int *d_mhalf_count = nullptr;   // [K][multi_count_stride] arrival counters per set
    int64_t multi_half_stride = 0, multi_count_stride = 0, multi_half_capacity = 0;
    double jit_compile_s = 0.0;     // hiprtc time spent for this batch (0: cache hit / none)
    rt_partition *part = nullptr;   // a partitioned batch (rt_sites_create_partitioned), owned
};

// ---- internal entry points ---------------------------------------------------------

void rt_time_begin(rt_ctx *ctx, int kernel, const char *name, hipEvent_t *start);
void rt_time_end(rt_ctx *ctx, int kernel, hipEvent_t start);
// a second kernel inside a launch that is being sampled (ctx->ev_start set): its own pair of
// events in its own slot; false = not timed (a, b stay null)
bool rt_time_extra_begin(rt_ctx *ctx, int kernel, const char *name, hipEvent_t *a, hipEvent_t *b);
void rt_time_extra_end(rt_ctx *ctx, int kernel, hipEvent_t a, hipEvent_t b);

// the reduction a launch may carry in one extra workgroup (partial == nullptr: none)
struct rt_reduce_args {
    const double *partial = nullptr;   // [npartials][2]
    long npartials = 0;
    double *totals = nullptr;          // [3]
    double nsites = 0.0;
};
// The root combine of a root-halves batch that the eight-wave 49..64-state expm launch may carry
// in its waves 4..7, which idle until the first barrier (halfbuf == nullptr: none).  The
// arguments of prune_mfma_combine_kernel / rt_jit_combine, plus the batch's layout of partial
// sums: wave_slots entries per tile (4: the interpreter's, 1: the tree-specialised kernels').
struct rt_combine_args {
    const double *halfbuf = nullptr;   // [tile][half][k-step][lane]
    const double *obs = nullptr;       // [tile][K][KP][64][2]
    int K = 0, KP = 0, kroot = -1;     // kroot: stream position of the root's observation, or -1
    const double *root_w = nullptr;
    int n = 0;
    double *loglik = nullptr;
    int *status = nullptr;
    double *partial = nullptr;
    long nsites = 0, nblocks16 = 0;
    int wave_slots = 1;
};
// How a carrying launch of G matrix workgroups deals the tiles: idle wave k (0..3) of workgroup
// wg finishes tile wg + k G -- one round, so a batch of more than 4 G tiles is not carried.
// -> the tile, or -1 (no tile for this wave)
__host__ __device__ inline long rt_carry_tile(long wg, int k, long G, long nblocks16)
{
    const long t = wg + (long)k * G;
    return t < nblocks16 ? t : -1;
}
// The whole rule, for the host (and exported as rt_carry_combine_deal for the tests): may a
// launch of G matrix workgroups carry the combine of a batch of nt row tiles per site tile and
// nblocks16 site tiles?  Only NT = 4 root halves, plain (no rescaling, no partition, no rate-set
// axis), all tiles in one round.  With tile_of (4 G entries) non-null: tile_of[4 wg + k].
inline bool rt_carry_combine_plan(int64_t nt, int64_t nblocks16, int64_t G, bool halves, bool rescale,
                                  bool partitioned, bool multi, int64_t *tile_of = nullptr)
{
    const bool ok = nt == 4 && halves && !rescale && !partitioned && !multi && G >= 1 &&
                    nblocks16 >= 1 && nblocks16 <= 4 * G;
    if (ok && tile_of)
        for (int64_t wg = 0; wg < G; ++wg)
            for (int k = 0; k < 4; ++k) tile_of[4 * wg + k] = rt_carry_tile((long)wg, k, (long)G, (long)nblocks16);
    return ok;
}
// expm.hip: the number of matrix workgroups G of the launch rt_launch_expm would make for these
// arguments if that launch is of the carrying kernel (eight waves, 49..64 states), else 0
int64_t rt_expm_carry_groups(rt_ctx *ctx, int64_t n, int64_t count, bool with_reduce, bool quad);
// expm_wide.hip: the LDS-resident Taylor kernel for 64 < n <= 128 (scratch: ctx->d_expm_scratch)
int rt_expm_wide_launch(rt_ctx *ctx, int nt, bool split2, size_t grid, int64_t n, const double *d_Q,
                        const int *d_qidx, const double *d_t, double *d_P, int *d_info,
                        const int *d_step_of_node, int frag_kind, double *d_Pfrag,
                        const rt_reduce_args &red);
// variant_count > 0: the kernel variant (one or two workgroups per matrix) is chosen as for
// that many matrices, whatever `count` is (K rate sets in one launch: each set's matrices are
// those of a launch over the set alone, bit for bit)
int rt_launch_expm(rt_ctx *ctx, int64_t n, int64_t count, const double *d_Q,
                   const int32_t *d_qidx, const double *d_t, double *d_P,
                   int32_t *d_info, const int32_t *d_step_of_node, int frag_kind,
                   double *d_Pfrag, const rt_reduce_args *fused_reduce = nullptr,
                   double *d_Pquad = nullptr, int64_t variant_count = 0,
                   const rt_combine_args *carried_combine = nullptr);
// spectral.hip: P_e = A diag(exp(lam t_e)) B per edge, outputs as rt_launch_expm's
int rt_launch_spectral(rt_ctx *ctx, int64_t n, int64_t count, const double *d_A,
                       const double *d_lam, const double *d_B, const double *d_D,
                       const int32_t *d_qidx, const double *d_t, double *d_P, int32_t *d_info,
                       const int32_t *d_step_of_node, int frag_kind, double *d_Pfrag,
                       const rt_reduce_args *fused_reduce = nullptr, double *d_Pquad = nullptr);
// the pending reduction, handed to the next expm launch (-> true) ...
bool rt_take_pending_reduce(rt_ctx *ctx, rt_reduce_args *out);
// ... or launched on its own now (no-op when nothing is pending)
int rt_flush_reduce(rt_ctx *ctx);
// The pending combine, handed to an expm launch of G matrix workgroups that also carries the
// reduction *red (partial == nullptr: none) -> true; false: not this launch (nothing pending,
// too many tiles for G, RAOTEH_CARRY_COMBINE=0), and then it has been launched on its own.
// *taken: the batch (the caller launches, then calls rt_carried_combine_done with it), or null.
int rt_take_pending_combine(rt_ctx *ctx, int64_t G, const rt_reduce_args *red, rt_combine_args *out,
                            struct rt_sites **taken);
int rt_carried_combine_done(rt_ctx *ctx, struct rt_sites *s, bool launched);
// the pending combine launched on its own now; its batch's reduction becomes the pending one
int rt_flush_combine(rt_ctx *ctx);
// Everything pending, with the stand-alone kernels: the combine, then the reduction.  Whoever
// reads or replaces the per-site results, the partial sums, the totals or the half buffer of a
// batch, or what a pending combine reads (root distribution, observations), calls this first.
int rt_flush_pending(rt_ctx *ctx);
// ... if any of it belongs to batch s
int rt_flush_pending_of(rt_ctx *ctx, const struct rt_sites *s);
// A timed launch: the runtime stamps the two events with the kernel's own begin and
// end (what rocprofv3's kernel trace reports), not with the stream position of an
// event record, which adds 2-3 us per pair.  Null events: a plain launch.
#define RT_LAUNCH_TIMED(ctx, kern, grid, block, lds, ...)                               \
    do {                                                                                \
        if ((ctx)->ev_start)                                                            \
            hipExtLaunchKernelGGL(kern, grid, block, lds, (ctx)->stream,                \
                                  (ctx)->ev_start, (ctx)->ev_stop, 0, __VA_ARGS__);     \
        else                                                                            \
            hipLaunchKernelGGL(kern, grid, block, lds, (ctx)->stream, __VA_ARGS__);     \
    } while (0)
int rt_launch_pfrag(rt_model *m);
int rt_model_pack_pcol(rt_model *m);            // (no-op without d_Pcol)
int rt_model_need_pcol(rt_model *m);            // allocate + fill from the current d_P
// the leaf-column tables of `sets` rate sets, set k from d_P + k * P_stride to d_Pcol + k * pcol_stride
int rt_pack_pcol_sets(rt_model *m, int64_t sets, const double *d_P, int64_t P_stride, double *d_Pcol,
                      int64_t pcol_stride);
// The tables a pruning launch reads and the per-site outputs it writes, when they are not the
// model's and the batch's own (rt_step_multi: one rate set's tables, that set's output slices).
// The observations, the root weights, the programs and the scratch of the batch stay its own.
struct rt_prune_view {
    const double *P = nullptr, *Pfrag = nullptr, *Pquad = nullptr, *Pcol = nullptr;
    double *loglik = nullptr;
    int32_t *status = nullptr;
    double *partial = nullptr;
    // a partitioned batch (rt_step_partitioned): the tables above are set 0's, granule g of the
    // batch reads those of set granule_set[g], the per-set strides (doubles) further on
    const int32_t *granule_set = nullptr;
    int64_t frag_stride = 0, pcol_stride = 0;
    // rt_step on a root-halves batch whose combine the next expm launch can carry: the launcher
    // records the batch as rt_ctx::pending_combine instead of launching the combine kernel
    bool defer_combine = false;
};
// prune.hip: sites per granule of the lane family's VGPR-ring kernel on this model's tree (the
// workgroup's span: 256 with the transition table staged in LDS, else 64)
int64_t rt_lane_reg_granule(const rt_model *m);
// partition.hip: what follows the pruning launch of a partitioned batch, asynchronous on the
// context's stream -- per set a fixed-order two-stage sum over the slot-ordered results (pads
// masked), the batch totals, and the results gathered into caller order
int rt_partition_stage1_blocks(int64_t longest_run);
int64_t rt_partition_totals_doubles(int64_t nsets, int nblocks);
int rt_partition_reduce_launch(rt_ctx *ctx, const rt_partition *part, const double *d_loglik,
                               const int32_t *d_status, const double *d_weights,
                               double *d_batch_totals);
// multi.hip: K fixed-order reductions (the arithmetic of rt_flush_reduce's kernel per set) and
// the weighted sums, asynchronous on the context's stream; the per-site mixture over the sets
int64_t rt_multi_totals_doubles(int64_t K, int64_t nsites);   // doubles behind d_totals
int rt_multi_reduce_launch(rt_ctx *ctx, int64_t K, const double *d_partial, int64_t npartials,
                           const double *d_loglik, const int32_t *d_status, int64_t padded,
                           int64_t nsites, const double *d_weights, double *d_totals,
                           double *d_wsums);
int rt_multi_mixture_launch(rt_ctx *ctx, int64_t K, const double *d_logc, const double *d_loglik,
                            const int32_t *d_status, int64_t padded, int64_t nsites,
                            const double *d_weights, double *d_out, int32_t *d_out_status,
                            double *d_partial, double *d_totals);
// fuse_expm: the pruning launch computes the transitions from the resident rates itself
// (batches with jit_fused only) and carries the pending reduction
// view: the launch reads / writes these instead (no reduction follows, nothing is deferred)
int rt_launch_prune(rt_model *m, rt_sites *s, bool defer_reduce = false, bool fuse_expm = false,
                    const struct rt_prune_view *view = nullptr);
// what such a launch is handed besides the pruning arguments
struct rt_fuse_args {
    rt_reduce_args red;     // partial == nullptr: nothing carried
    bool expm = false;      // compute the transitions (else copy the resident table)
};
// jit.hip
std::string rt_jit_lane_source(const std::vector<rt_op> &ops, int n, int K, int D, int LA,
                               int S, int WG, int compact = 0, bool fuse = false);
std::string rt_jit_mfma_source(const std::vector<rt_op> &ops, int n, int K, int T, int D, int LA,
                               bool quad = false, int sparse = 0);
// (sparse: 0 dense leaf vectors, 1 one observed state per leaf, 2 one or two allowed states)
std::string rt_jit_mfma_split_source(const std::vector<rt_op> &ops, int n, int K, int T, int D,
                                     int LA, int sparse = 0);
bool rt_jit_fold_enabled();
std::string rt_jit_mfma_split_pipelined_source(const std::vector<rt_op> &ops, int n, int K, int T,
                                               int D, int LA, bool halves = false,
                                               int sparse = 0, bool multi = false,
                                               bool teams = false);
// the two-team form of that generator (eight waves per workgroup) exists for these parameters
bool rt_jit_teams_possible(int n, int T, int sparse);
// RAOTEH_JIT_TEAMS: -1 not set (the policy decides), 0 / 1 forced
int rt_jit_teams_env();
// steps of the two root programs the halves form would run (0, 0: the root has < 2 children)
void rt_jit_root_halves(const std::vector<rt_op> &ops, int *stepsA, int *stepsB);
// the cut itself: A = the subtrees of all children of the root but the last, B = the last
// child's subtree, each followed by the root's step (both contiguous runs of `ops`)
bool rt_split_at_root(const std::vector<rt_op> &ops, std::vector<rt_op> *A, std::vector<rt_op> *B);
// another kernel of the module `fn` came from (the halves form's rt_jit_combine)
int rt_jit_companion(const rt_ctx *ctx, void *fn, const char *name, void **out);
int rt_jit_get(rt_ctx *ctx, const std::string &src, void **fn, bool mfma = false,
               double *compile_s = nullptr);
// background compilation (jit.hip): a host thread of this process works through candidate
// sources (the first that compiles without scratch wins) and leaves the kernel in the
// per-context cache; rt_jit_job_done polls (or joins), rt_jit_join_all before the context goes
std::shared_ptr<rt_jit_job> rt_jit_start(rt_ctx *ctx, std::vector<std::string> sources, bool mfma);
bool rt_jit_job_done(rt_jit_job *job, bool wait);
void rt_jit_job_result(rt_jit_job *job, int *rc, int *chosen, double *seconds, std::string *error);
void rt_jit_join_all(const rt_ctx *ctx);
int rt_jit_jobs_pending();
// (ctx, src): 1 compiled and usable, -1 compiled and rejected, 0 unknown (no reference taken)
int rt_jit_cached(const rt_ctx *ctx, const std::string &src);
// api.hip: swap the finished background kernel of a batch in (wait: join the job first)
int rt_sites_jit_poll(rt_sites *s, bool wait);
void rt_jit_ref(const rt_ctx *ctx, void *fn, int delta);
// every freshly compiled kernel is run once against the interpreter kernel on a probe
// batch before a user batch may launch it (api.hip verify_jit_kernel): 0 = not yet,
// 1 = verified; rt_jit_set_verified(false) rejects the kernel for good
int rt_jit_verified(const rt_ctx *ctx, void *fn);
void rt_jit_set_verified(const rt_ctx *ctx, void *fn, bool ok);
void rt_jit_release(const rt_ctx *ctx);
int rt_jit_read_global(const rt_ctx *ctx, void *fn, const char *name, void *dst, size_t bytes);
int rt_launch_prune_jit(rt_model *m, rt_sites *s, const rt_fuse_args *fuse = nullptr,
                        const struct rt_prune_view *view = nullptr);
// one launch for all K rate sets of a split-M batch whose multi-form kernel is s->multi_fn:
// set k reads Pfrag + k s_table (Pcol + k s_pcol) and writes loglik / status + k s_site,
// partial + k s_partial (half + k s_half, counters + k s_count)
struct rt_multi_launch {
    int64_t K = 0;
    const double *Pfrag = nullptr, *Pcol = nullptr;
    double *loglik = nullptr;
    int32_t *status = nullptr;
    double *partial = nullptr, *half = nullptr;
    int *counters = nullptr;
    long s_table = 0, s_site = 0, s_partial = 0, s_half = 0, s_count = 0, s_pcol = 0;
};
int rt_launch_prune_jit_multi(rt_model *m, rt_sites *s, const rt_multi_launch &a);
// a batch that runs the interpreter kernels only (no tree-specialised kernel is compiled)
int rt_sites_create_interpreter(rt_model *m, int64_t nsites, int kind, int64_t nobs,
                                const int64_t *obs_nodes, const void *data, rt_sites **out);
// drops what rt_expectation_weights_mfma keeps between calls (rt_ctx_destroy)
void rt_expect_cache_release(rt_ctx *ctx);
// expect.hip: assemble / exponentiate / contract the Frechet blocks on device-resident operands
int rt_frechet_statistics_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dQ,
                                 const int32_t *dqidx, const double *dt, const double *dW,
                                 double *dB, double *dE, double *dscale, const double *dones,
                                 const int32_t *dident, double *ddwell, double *dtrans);
// ... its two halves for a caller that wants the derivatives themselves (branch_expect.hip): the
// block exponentials without the contraction, then dG[e][a][b] = t_e L(t_e Q_e, C_e)[a][b] for
// dW[e] = C_e^T
// (variant_count > 0: the exponential's kernel variant is chosen as for that many edges, as
// rt_launch_expm's -- the edges of K rate sets in one launch, each set's as in a launch of its own)
int rt_frechet_blocks_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dQ,
                             const int32_t *dqidx, const double *dt, const double *dW, double *dB,
                             double *dE, double *dscale, const double *dones, const int32_t *dident,
                             int64_t variant_count = 0);
int rt_frechet_extract_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dt,
                              const double *dE, const double *dscale, double *dG);
// frechet_wide.hip: the same for 64 < n <= 128 by the pair recurrence (no order-2n block);
// dS: rt_frechet_wide_scratch_doubles(n, nedges) doubles, dinfo (optional) {degree, squarings}
size_t rt_frechet_wide_scratch_doubles(int64_t n, int64_t nedges);
int rt_frechet_wide_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dQ,
                           const int32_t *dqidx, const double *dt, const double *dW, double *dS,
                           double *dscale, int32_t *dinfo, double *ddwell, double *dtrans);
int rt_frechet_wide_pairs_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dQ,
                                 const int32_t *dqidx, const double *dt, const double *dW, double *dS,
                                 double *dscale, int32_t *dinfo);
int rt_frechet_wide_extract_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dt,
                                   const double *dS, const double *dscale, double *dG);
// ... and what rt_expect_step keeps with a model (rt_model_destroy)
void rt_expect_state_release(rt_model *m);
// passes.hip: the lane form (n <= 4) of rt_expect_step's passes.  rt_expect_lane_take: its pieces
// of the call's scratch; then W and the status (cleared by the caller) on the device,
// asynchronous on the context's stream
struct rt_expect_lane_scratch { size_t o_L = 0, o_part = 0; };
rt_expect_lane_scratch rt_expect_lane_take(const rt_model *m, const rt_sites *s, post_plan *plan);
int rt_expect_lane_resident(rt_model *m, rt_sites *s, unsigned char *scratch,
                            const rt_expect_lane_scratch &at, double *d_W, int *d_status);
void rt_expect_lane_release(rt_model *m);
// expect_mfma.hip: P^T as A fragments in step order, T[step][m][q][lane][2] (NT row tiles,
// KP k-step pairs), asynchronous on the context's stream
int rt_launch_pack_pt(rt_ctx *ctx, int n, int NT, int KP, int nops, const int *d_step_node,
                      const double *d_P, double *d_PT);
// ... and P itself in the same form (the products P x of place.hip)
int rt_launch_pack_p(rt_ctx *ctx, int n, int NT, int KP, int nops, const int *d_step_node,
                     const double *d_P, double *d_PA);
// a split-M interpreter batch over the resident observations of `src` (api.hip); of a
// partitioned batch: over its slots, launched through a view with the batch's granule_set
int rt_sites_twin_interpreter(rt_sites *src, rt_sites **out);
// api.hip: the K (nnodes - 1) exponentials again from the resident rate sets, every table of the
// sets rewritten (what rt_step_partitioned does with recompute_transitions)
int rt_rate_sets_recompute(rt_model *m);
// passes.hip: the context's grow-only device scratch (ctx->d_scratch) holds at least `bytes`
// afterwards
int rt_scratch_reserve(rt_ctx *ctx, size_t bytes);
// expectation path on the matrix pipe (expect_mfma.hip); RT_ERR_UNSUPPORTED = not this case
int rt_expectation_weights_mfma(rt_ctx *ctx, int64_t nnodes, int64_t n, int64_t nsites,
                                const int64_t *idx, const int64_t *ptr, const double *esd,
                                const double *root_distn, int64_t nobs, const int64_t *obs_nodes,
                                int kind, const void *data, const double *site_weights,
                                double *edge_weights, int32_t *status);
int rt_sites_pack(rt_sites *s, int kind, const int64_t *obs_order,
                  const void *data);
int rt_sites_pack_device(rt_sites *s, int kind, const void *d_in, const int *d_src);

static inline int64_t rt_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
// doubles per step of the quad-block table (rt_model::d_Pquad): ceil(n/4)^2 blocks of 16,
// rounded up to whole 1 KiB wave loads (64 lanes x 16 bytes)
__host__ __device__ static inline int rt_quad_stride(int n)
{
    const int ks = (n + 3) / 4;
    return (ks * ks * 16 + 127) / 128 * 128;
}
