// scorer.hip - the selection loop behind the C ABI: ipsx_scan* / ipsx_scan_persistent* / ipsx_scan_gate / ipsx_publish_rows
// pick the kernel a shape takes (scan_fast.hip, scan_cam.hip, scan_mnist.hip, scan_large.hip) and own the process-wide switches.
// (Round 6: the logits live in logits.hip, scores / top-M in topm.hip, shared device code in scan_common.h.)
//
// Reference: MultiHeadCrossAttention.get_attn (architecture/transformer.py:71-83),
// ScaledDotProductAttention.compute_attn (:29-34), Transformer.get_scores (:143-148),
// IPSNet.score_and_select (architecture/ips_net.py:136-155) and the chunk loop of
// IPSNet.ips (:213-241).
//
// A patch's logits  l[h,t] = (q_w q)[t,h,:]/sqrt(Dk) . (k_w (emb+pos))[h,:]  depend on
// that patch alone; only the softmax denominator depends on the candidate set.  So
//   logits_kernel  computes them once per patch (K projection on the fp32 matrix
//                  cores, q.k reduction from LDS), and
//   scan_fast_kernel / scan_large_kernel  replay the reference loop on those cached
//                  logits with ONE workgroup per image: per-(h,t) softmax statistics by
//                  wavefront reductions, mean over heads then tokens, rank, keep the
//                  top M - no host round trips.
// Arithmetic order is the oracle's (oracle/ips_oracle.cpp orc_logits,
// orc_scores_from_logits, orc_topm).
//
// Algorithmic bytes of the scan: R*4 bytes of logits per patch (R = H*n_token), read
// once per iteration it takes part in.

#include <algorithm>
#include <cstdlib>

#include "scan_common.h"

namespace ipsx {

int g_tie_order = 1;     // 0 canonical; 1 (default) torch.topk's order where bit-identical candidates tie; 2 wherever scores tie
int g_persist_wait_ms = 50;         // ipsx_set_persistent_wait_ms: longest wait of a persistent loop / its gate without progress
bool g_scan_generic = false;        // diagnostic (ipsx_dbg_scan_generic): every shape through scan_large_kernel
bool g_replay_stamps_on = false;    // diagnostic (ipsx_dbg_replay_stamps): the replay's phases are stamped from the first read on
bool g_scan_team_trunc = true;      // diagnostic (ipsx_dbg_scan_team_trunc)
int g_scan_team = -1;               // diagnostic (ipsx_dbg_scan_team): workgroups per image of scan_large_team_kernel (-1: default)
bool g_scan_direct = true;          // diagnostic (ipsx_dbg_scan_direct): 0 = scan_large_kernel's five generic passes for every shape
bool g_scan_r8 = true;              // diagnostic (ipsx_dbg_scan_r8): 0 sends the shape of scan_cam_kernel through scan_fast_kernel
bool g_scan_mnist = true;           // diagnostic (ipsx_dbg_scan_mnist): 0 sends the shape of scan_mnist_kernel through scan_fast_kernel
bool g_scan_logits = true;          // diagnostic (ipsx_dbg_scan_logits): 0 = ipsx_scan_range_logits enqueues logits launches and loop launches
unsigned long long* g_scan_stamps = nullptr;   // diagnostic only (ipsx_dbg_scan_stamps)

// Diagnostic (ipsx_dbg_persist_log; tools/soak.py): what the gate and the resident loops saw, on the 100 MHz clock -
// [0] gate launches, [1] longest gate wait (ticks), [2] gate waits that ran into their bound, [3] start of the last gate,
// [4] the moment the last loop became resident, [5] loops that gave up waiting for rows, [6] start of the slowest gate,
// [7] the moment the loop it waited for became resident (0: not before the gate gave up)
__device__ unsigned long long g_persist_log[8];


unsigned long long* persist_log() {
    static unsigned long long* p[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!p[dev]) {
        void* q = nullptr;
        if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_persist_log)) == hipSuccess) p[dev] = static_cast<unsigned long long*>(q);
    }
    return p[dev];
}

// What every entry point of the loop has, in the order the C ABI names it; what an entry has beyond that it names itself.
static ScanCall scan_call(const float* logits, int b, int64_t n, int m, int i, int h, int n_token, int64_t* mem_idx,
                          float* mem_score, int32_t* tie_flag, void* stream) {
    ScanCall c;
    c.logits = logits; c.b = b; c.n = n; c.m = m; c.i = i; c.h = h; c.n_token = n_token;
    c.mem_idx = mem_idx; c.mem_score = mem_score; c.tie_flag = tie_flag; c.stream = stream;
    return c;
}

// the whole loop over n rows (callers have checked n > m, i > 0)
static void whole_loop(ScanCall& c) { c.it_begin = 0; c.it_end = (c.n - c.m + c.i - 1) / c.i; }

// THE check of a call before any launcher sees it: the sizes and the iteration range, and the combinations no kernel is
// built for - without this they would be served as if the logits were packed.  (No entry point builds one of those today.)
static int validate_scan_call(const ScanCall& c) {
    IPSX_REQUIRE(c.logits && c.mem_idx, "scan: null pointer");
    IPSX_REQUIRE(c.b > 0 && c.m > 0 && c.i > 0 && c.h > 0 && c.n_token > 0, "scan: bad sizes");
    IPSX_REQUIRE(c.n > c.m, "scan: needs more patches (%lld) than memory slots (%d)", (long long)c.n, c.m);
    IPSX_REQUIRE(c.n < ((int64_t)1 << 31), "scan: too many patches");
    IPSX_REQUIRE(c.it_begin >= 0 && c.it_begin <= c.it_end && c.it_end <= (c.n - c.m + c.i - 1) / c.i,
                 "scan: iteration range [%lld, %lld) outside the loop", (long long)c.it_begin, (long long)c.it_end);
    if (c.rows == Rows::Packed) return IPSX_OK;
    IPSX_REQUIRE(!c.ready && !c.cond && !g_scan_stamps,
                 "scan: only packed logits are waited for (persistent), launched conditionally or stamped");
    IPSX_REQUIRE(c.table_rows > 0 && c.table_rows < ((int64_t)1 << 31), "scan: a table of %lld rows", (long long)c.table_rows);
    if (rows_per_slide(c.rows)) {
        IPSX_REQUIRE(c.slide_table, "scan: slides without their table");
        IPSX_REQUIRE(c.workgroups <= 0 || c.workgroups >= c.b, "scan: slides of different lengths take a workgroup each");
    }
    return IPSX_OK;
}

// THE kernel choice of every entry point.
static int dispatch_scan(const ScanCall& c) {
    IPSX_TRY(validate_scan_call(c));
    if (c.it_begin == c.it_end) return IPSX_OK;
    const FastPlan fp = scan_fast_plan(c.m, c.i, c.h, c.n_token);
    // every shape the LDS-resident loops do not cover - other head / token counts, candidate sets beyond the LDS (the
    // reference's shipped CAMELYON configuration: M = I = 5000): scan_large_kernel (forced generic: plain launches only)
    if (!fp.ok || (g_scan_generic && !c.ready && !c.cond)) return launch_scan_large(c);
    // BASELINE configs[3] (8 heads, one token, M = I = 256): the specialised loop
    if (g_scan_r8 && scan_cam_shape(c.m, c.i, c.h, c.n_token)) return launch_scan_cam(c);
    // BASELINE configs[1] / [2] (8 heads, 4 tokens, M = I = 64): the specialised loop - plain, conditional and persistent
    // launches of one workgroup per image on packed logits; every other layout (never a ragged call, then) and the stamped
    // diagnostic build stay on scan_fast_kernel
    if (g_scan_mnist && scan_mnist_shape(c.m, c.i, c.h, c.n_token) && c.rows == Rows::Packed &&
        (c.workgroups <= 0 || c.workgroups >= c.b) && g_scan_stamps == nullptr)
        return launch_scan_mnist(c);
    return launch_scan_fast(c, fp);
}

}  // namespace ipsx

using namespace ipsx;

IPSX_API int ipsx_scan(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                       int64_t* mem_idx, float* mem_score, int32_t* tie_flag, void* workspace, size_t workspace_bytes,
                       void* stream) {
    IPSX_REQUIRE(n > m && i > 0, "scan: needs more patches (%lld) than memory slots (%d)", (long long)n, m);
    if (tie_flag && hipMemsetAsync(tie_flag, 0, sizeof(int32_t) * (size_t)std::max(b, 0), as_stream(stream)) != hipSuccess)
        return fail(IPSX_EHIP, "scan: memset failed");
    return ipsx_scan_range(logits, b, n, m, i, h, n_token, 0, (n - m + i - 1) / i, mem_idx, mem_score, tie_flag,
                           workspace, workspace_bytes, stream);
}

IPSX_API int ipsx_scan_range(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                             int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                             int32_t* tie_flag, void* workspace, size_t workspace_bytes, void* stream) {
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    c.it_begin = it_begin; c.it_end = it_end;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return dispatch_scan(c);
}

// ipsx_scan_range on logits that sit in a table of fixed capacity: image k's rows start k * logits_bstride_rows rows behind
// image 0's, n of them are candidates (a stream's candidate table: n changes from feed to feed, the capacity does not).
IPSX_API int ipsx_scan_range_strided(const float* logits, int64_t logits_bstride_rows, int b, int64_t n, int m, int i, int h,
                                     int n_token, int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                                     int32_t* tie_flag, void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(logits_bstride_rows >= n && logits_bstride_rows < ((int64_t)1 << 31),
                 "scan_range_strided: %lld rows between the images hold %lld candidates (fewer than 2^31)",
                 (long long)logits_bstride_rows, (long long)n);
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    c.it_begin = it_begin; c.it_end = it_end;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    if (logits_bstride_rows != n) {                        // (a full table is packed logits: every kernel of ipsx_scan_range)
        c.rows = Rows::Strided;
        c.table_rows = logits_bstride_rows;
    }
    return dispatch_scan(c);
}

// ipsx_scan on slides of different lengths: slide k's logits are rows [row_offsets[k], row_offsets[k + 1]) of ONE packed
// (total, R) table, the offsets b + 1 int64 on the device.  One plain launch of one workgroup per slide - the Rows::Offsets
// instantiation of the loop kernel the shape takes (never scan_mnist_kernel, never a team) -, each replaying the loop of
// ipsx_scan for its slide alone: mem_idx (b, m) is slide-local.  n_max (the longest slide) and total are the caller's
// host-side knowledge; every slide has more than m rows (a slide that has not, or that leaves the table, is left untouched).
IPSX_API int ipsx_scan_ragged(const float* logits, const int64_t* row_offsets, int b, int64_t n_max, int64_t total, int m,
                              int i, int h, int n_token, int64_t* mem_idx, float* mem_score, int32_t* tie_flag,
                              void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(logits && row_offsets && mem_idx, "scan_ragged: null pointer");
    IPSX_REQUIRE(b > 0 && m > 0 && i > 0 && h > 0 && n_token > 0, "scan_ragged: bad sizes");
    IPSX_REQUIRE(n_max > m, "scan_ragged: needs more patches per slide (longest: %lld) than memory slots (%d)", (long long)n_max, m);
    IPSX_REQUIRE(total >= n_max && total <= (int64_t)b * n_max && total < ((int64_t)1 << 31),
                 "scan_ragged: %lld rows in all (fewer than 2^31) for %d slides of at most %lld", (long long)total, b, (long long)n_max);
    if (tie_flag && hipMemsetAsync(tie_flag, 0, sizeof(int32_t) * (size_t)b, as_stream(stream)) != hipSuccess)
        return fail(IPSX_EHIP, "scan_ragged: memset failed");
    ScanCall c = scan_call(logits, b, n_max, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    whole_loop(c);
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.rows = Rows::Offsets; c.slide_table = row_offsets; c.table_rows = total;
    return dispatch_scan(c);
}

// ipsx_scan_ragged on slides that lie anywhere in ONE (rows_total, R) table: spans (b, 2) int64 on the device, slide k's first
// row and row count (the blocks of a ragged stream's logits table, IPSNet.ips_ragged_stream: the counts change from feed to
// feed, the blocks do not move).  The Rows::Spans instantiation of the loop kernel the shape takes, one workgroup per slide; a
// slide whose count is not above m, or whose span leaves the table, is left untouched in all three outputs - tie_flag
// included, so nothing is cleared here.  n_max: the caller's bound on the counts (dispatch and the < 2^31 checks only).
IPSX_API int ipsx_scan_ragged_spans(const float* logits, const int64_t* spans, int b, int64_t n_max, int64_t rows_total, int m,
                                    int i, int h, int n_token, int64_t* mem_idx, float* mem_score, int32_t* tie_flag,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(logits && spans && mem_idx, "scan_ragged_spans: null pointer");
    IPSX_REQUIRE(b > 0 && m > 0 && i > 0 && h > 0 && n_token > 0, "scan_ragged_spans: bad sizes");
    IPSX_REQUIRE(n_max > m, "scan_ragged_spans: needs more patches per slide (longest: %lld) than memory slots (%d)", (long long)n_max, m);
    IPSX_REQUIRE(rows_total >= n_max && rows_total < ((int64_t)1 << 31),
                 "scan_ragged_spans: a table of %lld rows (fewer than 2^31) for slides of at most %lld", (long long)rows_total, (long long)n_max);
    ScanCall c = scan_call(logits, b, n_max, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    whole_loop(c);
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.rows = Rows::Spans; c.slide_table = spans; c.table_rows = rows_total;
    return dispatch_scan(c);
}

IPSX_API size_t ipsx_scan_workspace_bytes(int b, int m, int i, int h, int n_token) {
    if (b <= 0 || m <= 0 || i <= 0 || h <= 0 || n_token <= 0) return 0;
    if (scan_fast_plan(m, i, h, n_token).ok && !g_scan_generic) return 0;
    return (size_t)b * scan_large_ws_per_image(m, i, h, n_token);
}

IPSX_API int ipsx_scan_workgroups_per_image(int b, int m, int i, int h, int n_token) {
    if (b <= 0 || m <= 0 || i <= 0 || h <= 0 || n_token <= 0) return 0;
    if (scan_fast_plan(m, i, h, n_token).ok && !g_scan_generic) return 1;
    return scan_large_team(b, m, i, h, n_token);
}

__global__ void publish_rows_kernel(int* ready, int value) {
    __hip_atomic_store(ready, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

IPSX_API int ipsx_scan_persistent_supported(int m, int i, int h, int n_token) {
    if (m <= 0 || i <= 0 || h <= 0 || n_token <= 0) return 0;
    return scan_fast_plan(m, i, h, n_token).ok ? 1 : 0;
}

IPSX_API int ipsx_scan_persistent(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                                  int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const int32_t* ready,
                                  int32_t ready_per_image, int32_t* status, void* stream) {
    IPSX_REQUIRE(ready && status, "scan_persistent: needs the progress word(s) and the status word");
    IPSX_REQUIRE(n > m && i > 0, "scan: needs more patches (%lld) than memory slots (%d)", (long long)n, m);
    IPSX_REQUIRE(ipsx_scan_persistent_supported(m, i, h, n_token), "scan_persistent: shape not covered (use ipsx_scan_range)");
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    whole_loop(c);
    c.ready = ready; c.ready_stride = ready_per_image ? 1 : 0; c.status = status;
    return dispatch_scan(c);
}

IPSX_API int ipsx_scan_persistent_groupable(int m, int i, int h, int n_token) {
    return g_scan_r8 && scan_cam_shape(m, i, h, n_token) ? 1 : 0;
}

IPSX_API int ipsx_scan_persistent_on(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                                     int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const int32_t* ready,
                                     int32_t ready_per_image, int32_t* status, int workgroups, void* stream) {
    IPSX_REQUIRE(ready && status, "scan_persistent: needs the progress word(s) and the status word");
    IPSX_REQUIRE(n > m && i > 0, "scan: needs more patches (%lld) than memory slots (%d)", (long long)n, m);
    IPSX_REQUIRE(ipsx_scan_persistent_supported(m, i, h, n_token), "scan_persistent: shape not covered (use ipsx_scan_range)");
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    whole_loop(c);
    c.ready = ready; c.ready_stride = ready_per_image ? 1 : 0; c.status = status;
    c.workgroups = workgroups;
    return dispatch_scan(c);
}

// The persistent loop for EVERY shape ipsx_scan covers - candidate sets beyond the LDS take the workspace of ipsx_scan
// (ipsx_scan_workspace_bytes; scan_large_kernel waits for its rows like the LDS-resident loops do) - and the conditional
// recovery launch with a workspace.
IPSX_API int ipsx_scan_persistent_ws(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                                     int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const int32_t* ready,
                                     int32_t ready_per_image, int32_t* status, int workgroups, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(ready && status, "scan_persistent: needs the progress word(s) and the status word");
    IPSX_REQUIRE(n > m && i > 0, "scan: needs more patches (%lld) than memory slots (%d)", (long long)n, m);
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    whole_loop(c);
    c.ready = ready; c.ready_stride = ready_per_image ? 1 : 0; c.status = status;
    c.workgroups = workgroups;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return dispatch_scan(c);
}

IPSX_API int ipsx_scan_range_if_ws(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                                   int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                                   int32_t* tie_flag, const int32_t* cond, int32_t cond_mask, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    IPSX_REQUIRE(cond && cond_mask, "scan_range_if: needs the condition word and a mask");
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    c.it_begin = it_begin; c.it_end = it_end;
    c.cond = cond; c.cond_mask = cond_mask;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return dispatch_scan(c);
}

// one thread that holds its stream until every workgroup of the persistent scan is resident (bounded: ~0.5 s)
__global__ void scan_gate_kernel(const int* status, unsigned long long wait_ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool gave_up = false;
    while ((__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2) == 0) {
        __builtin_amdgcn_s_sleep(8);
        if (__builtin_amdgcn_s_memrealtime() - t0 > wait_ticks) { gave_up = true; break; }
    }
    const unsigned long long waited = __builtin_amdgcn_s_memrealtime() - t0;
    g_persist_log[0] += 1;
    g_persist_log[3] = t0;
    if (gave_up) g_persist_log[2] += 1;
    if (waited > g_persist_log[1]) {
        g_persist_log[1] = waited;
        g_persist_log[6] = t0;
        g_persist_log[7] = gave_up ? 0ull : __hip_atomic_load(&g_persist_log[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

IPSX_API int ipsx_scan_gate(const int32_t* status, void* stream) {
    IPSX_REQUIRE(status, "scan_gate: null pointer");
    scan_gate_kernel<<<dim3(1), dim3(1), 0, as_stream(stream)>>>(status, (unsigned long long)g_persist_wait_ms * 100000ull);
    return launched("scan_gate");
}

// One wavefront that holds its stream until a part of a counted trunk launch (ipsx_trunk_encode_parts) is complete:
// *done >= want.  Relaxed polls with a sleep between them, ONE acquire at the end.  Bounded WITHOUT PROGRESS: the clock
// restarts whenever the counter has moved, and a wait that sees none for wait_ticks sets `bit` in *status and returns - the
// caller's conditional launches (ipsx_logits_if, ipsx_scan_range_if) then redo what ran too early.
__global__ void part_wait_kernel(const int* done, int want, int* status, int bit, unsigned long long wait_ticks) {
    unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int last = __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (last < want) {
        __builtin_amdgcn_s_sleep(32);
        const int v = __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
        if (v != last) { last = v; t0 = t; }
        else if (t - t0 > wait_ticks) {
            __hip_atomic_fetch_or(status, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

IPSX_API int ipsx_part_wait(const int32_t* done, int32_t want, int32_t* status, int32_t bit, void* stream) {
    IPSX_REQUIRE(done && status && bit, "part_wait: needs the counter, the status word and a bit");
    part_wait_kernel<<<dim3(1), dim3(1), 0, as_stream(stream)>>>(done, want, status, bit,
                                                                 (unsigned long long)g_persist_wait_ms * 100000ull);
    return launched("part_wait");
}

IPSX_API int ipsx_publish_rows(int32_t* ready, int32_t value, void* stream) {
    IPSX_REQUIRE(ready, "publish_rows: null pointer");
    publish_rows_kernel<<<dim3(1), dim3(1), 0, as_stream(stream)>>>(ready, value);
    return launched("publish_rows");
}

IPSX_API int ipsx_scan_range_if(const float* logits, int b, int64_t n, int m, int i, int h, int n_token,
                                int64_t it_begin, int64_t it_end, int64_t* mem_idx, float* mem_score,
                                int32_t* tie_flag, const int32_t* cond, int32_t cond_mask, void* stream) {
    IPSX_REQUIRE(cond && cond_mask, "scan_range_if: needs the condition word and a mask");
    IPSX_REQUIRE(scan_fast_plan(m, i, h, n_token).ok, "scan_range_if: shapes of the LDS-resident loop only");
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    c.it_begin = it_begin; c.it_end = it_end;
    c.cond = cond; c.cond_mask = cond_mask;
    return dispatch_scan(c);
}

// ---- ipsx_scan_range_logits: a range of the loop whose launch computes its own logits (scan_mnist_kernel's prologue)
// The part table's arithmetic, on the host, before anything is launched: parts [0, n_parts) tile the rows [0, n) of an image in
// order (first[k] = rows[0] + ... + rows[k - 1]), the launch's parts [part_begin, part_end) are among them - none of them
// (part_begin == part_end) when the rows are an earlier launch's and the launch is there for its redo -, and the rows its
// iterations [it_begin, it_end) read - up to min(n, m + it_end * i) - end where part part_end - 1 ends at the latest (the
// rows in front of part_begin are an earlier launch's).
IPSX_API int ipsx_scan_logits_check(const ipsx_logits_part* parts, int n_parts, int part_begin, int part_end, int64_t n, int m,
                                    int i, int64_t it_begin, int64_t it_end) {
    IPSX_REQUIRE(parts && n_parts >= 1 && n_parts <= SCAN_LOGITS_PARTS, "scan_range_logits: 1 to %d parts (got %d)", SCAN_LOGITS_PARTS, n_parts);
    IPSX_REQUIRE(part_begin >= 0 && part_begin <= part_end && part_end <= n_parts, "scan_range_logits: parts [%d, %d) of %d", part_begin,
                 part_end, n_parts);
    IPSX_REQUIRE(m > 0 && i > 0 && n > m && n < ((int64_t)1 << 31), "scan_range_logits: more patches (%lld, fewer than 2^31) than memory slots (%d)",
                 (long long)n, m);
    int64_t at = 0;
    for (int k = 0; k < n_parts; ++k) {
        IPSX_REQUIRE(parts[k].rows > 0 && parts[k].rows <= n, "scan_range_logits: part %d has %lld rows per image", k, (long long)parts[k].rows);
        IPSX_REQUIRE(parts[k].first == at, "scan_range_logits: part %d starts at row %lld, the parts in front of it end at %lld", k,
                     (long long)parts[k].first, (long long)at);
        at += parts[k].rows;
    }
    IPSX_REQUIRE(at == n, "scan_range_logits: the parts hold %lld rows per image, an image has %lld", (long long)at, (long long)n);
    IPSX_REQUIRE(it_begin >= 0 && it_begin < it_end && it_end <= (n - m + i - 1) / i, "scan_range_logits: iteration range [%lld, %lld) outside the loop",
                 (long long)it_begin, (long long)it_end);
    const int64_t read_end = std::min<int64_t>(n, (int64_t)m + it_end * i);
    const int64_t have_end = part_end > 0 ? parts[part_end - 1].first + parts[part_end - 1].rows : 0;
    IPSX_REQUIRE(read_end <= have_end, "scan_range_logits: iterations up to %lld read rows up to %lld, the parts in front of part %d end at %lld",
                 (long long)it_end, (long long)read_end, part_end, (long long)have_end);
    return IPSX_OK;
}

// the checks the two entry points share: the tensors, the shape, the part table and the two ranges
static int scan_logits_checked(float* logits, int b, int64_t n, int m, int i, int h, int n_token, int64_t it_begin, int64_t it_end,
                               int64_t* mem_idx, const ipsx_logits_part* parts, int n_parts, int part_begin, int part_end, int d,
                               const float* pos, int64_t pos_bstride, const float* v_packed, const int32_t* redo, int32_t redo_mask) {
    IPSX_REQUIRE(logits && mem_idx && v_packed && b > 0, "scan_range_logits: null pointer");
    IPSX_REQUIRE(scan_mnist_shape(m, i, h, n_token), "scan_range_logits: 8 heads x 4 tokens, M = I = 64 (scan_mnist_kernel) only");
    IPSX_REQUIRE(d > 0 && d % 8 == 0, "scan_range_logits: embeddings of whole 8-float groups (d = %d)", d);
    IPSX_REQUIRE(!redo == !redo_mask, "scan_range_logits: the redo word and its mask go together");
    IPSX_TRY(ipsx_scan_logits_check(parts, n_parts, part_begin, part_end, n, m, i, it_begin, it_end));
    for (int k = 0; k < n_parts; ++k)
        IPSX_REQUIRE(parts[k].emb && (reinterpret_cast<uintptr_t>(parts[k].emb) & 15) == 0, "scan_range_logits: part %d's embeddings at a 16-byte address", k);
    IPSX_REQUIRE((reinterpret_cast<uintptr_t>(v_packed) & 15) == 0 && (reinterpret_cast<uintptr_t>(pos) & 15) == 0 && pos_bstride >= 0 &&
                 pos_bstride % 4 == 0, "scan_range_logits: the folded query and the positional table at 16-byte addresses");
    return IPSX_OK;
}

// the prologue's arguments of a checked call
static ScanLogits scan_logits_table(float* logits, const ipsx_logits_part* parts, int n_parts, int part_begin, int part_end, int d,
                                    const float* pos, int64_t pos_bstride, const float* v_packed, const int32_t* redo, int32_t redo_mask) {
    ScanLogits p = {};
    for (int k = 0; k < n_parts; ++k) { p.part[k].emb = parts[k].emb; p.part[k].rows = (int)parts[k].rows; p.part[k].first = (int)parts[k].first; }
    p.pos = pos; p.pos_bs = pos_bstride; p.vp = v_packed; p.out = logits; p.redo = redo; p.redo_mask = redo_mask;
    p.d = d; p.kgs = d / 8; p.n_parts = n_parts; p.part0 = part_begin; p.part1 = part_end;
    return p;
}

IPSX_API int ipsx_scan_range_logits(float* logits, int b, int64_t n, int m, int i, int h, int n_token, int64_t it_begin, int64_t it_end,
                                    int64_t* mem_idx, float* mem_score, int32_t* tie_flag, const ipsx_logits_part* parts, int n_parts,
                                    int part_begin, int part_end, int d, const float* pos, int64_t pos_bstride, const float* v_packed,
                                    const int32_t* redo, int32_t redo_mask, void* stream) {
    IPSX_TRY(scan_logits_checked(logits, b, n, m, i, h, n_token, it_begin, it_end, mem_idx, parts, n_parts, part_begin, part_end, d, pos,
                                 pos_bstride, v_packed, redo, redo_mask));
    const int r = h * n_token;
    if (!g_scan_logits) {
        // the launches this entry point replaces, one by one (tests, A/B): the parts' logits and the range; with a redo word,
        // the conditional logits of the other parts and the conditional loop from iteration 0 behind them
        for (int k = part_begin; k < part_end; ++k)
            IPSX_TRY(ipsx_logits(parts[k].emb, parts[k].rows * d, pos ? pos + parts[k].first * d : nullptr, pos_bstride, v_packed, b, parts[k].rows, d, r,
                                 logits + parts[k].first * r, n * r, stream));
        IPSX_TRY(ipsx_scan_range(logits, b, n, m, i, h, n_token, it_begin, it_end, mem_idx, mem_score, tie_flag, nullptr, 0, stream));
        if (!redo) return IPSX_OK;
        for (int k = 0; k < n_parts; ++k)
            if (k < part_begin || k >= part_end)
                IPSX_TRY(ipsx_logits_if(parts[k].emb, parts[k].rows * d, pos ? pos + parts[k].first * d : nullptr, pos_bstride, v_packed, b, parts[k].rows,
                                        d, r, logits + parts[k].first * r, n * r, redo, redo_mask, stream));
        return ipsx_scan_range_if(logits, b, n, m, i, h, n_token, 0, it_end, mem_idx, mem_score, tie_flag, redo, redo_mask, stream);
    }
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    c.it_begin = it_begin; c.it_end = it_end;
    IPSX_TRY(validate_scan_call(c));
    return launch_scan_mnist_logits(c, scan_logits_table(logits, parts, n_parts, part_begin, part_end, d, pos, pos_bstride, v_packed, redo, redo_mask));
}

// ipsx_scan_range_logits with the hand-over between two launches on different streams (ScanGate, scan_mnist.hip): the launch
// waits on the device for gate[k] >= gate_target behind its prologue, stores it_end to gate_publish[k] at its end, writes
// its final indices to mem_out - each of the three on its own or not at all.  Always scan_mnist_kernel's one launch: the
// launches ipsx_dbg_scan_logits(0) puts in its place have no such hand-over.
IPSX_API int ipsx_scan_range_logits_gate(float* logits, int b, int64_t n, int m, int i, int h, int n_token, int64_t it_begin,
                                         int64_t it_end, int64_t* mem_idx, float* mem_score, int32_t* tie_flag,
                                         const ipsx_logits_part* parts, int n_parts, int part_begin, int part_end, int d, const float* pos,
                                         int64_t pos_bstride, const float* v_packed, const int32_t* redo, int32_t redo_mask,
                                         const int32_t* gate, int32_t gate_target, int32_t* gate_publish, int32_t* status,
                                         int32_t status_bit, int64_t* mem_out, void* stream) {
    IPSX_TRY(scan_logits_checked(logits, b, n, m, i, h, n_token, it_begin, it_end, mem_idx, parts, n_parts, part_begin, part_end, d, pos,
                                 pos_bstride, v_packed, redo, redo_mask));
    IPSX_REQUIRE(gate ? gate_target > 0 && gate_target >= it_begin : gate_target == 0,
                 "scan_range_logits_gate: a gate goes with its target, the iteration the range resumes from or a later one (target %d, range from %lld)",
                 (int)gate_target, (long long)it_begin);
    IPSX_REQUIRE(gate ? status && status_bit : !status == !status_bit,
                 "scan_range_logits_gate: a gate needs the status word and a bit for a wait that gives up");
    IPSX_REQUIRE(it_end < ((int64_t)1 << 31), "scan_range_logits_gate: the iteration published is a 32-bit word");
    IPSX_REQUIRE(!mem_out || mem_out != mem_idx, "scan_range_logits_gate: mem_out is a buffer of its own");
    ScanCall c = scan_call(logits, b, n, m, i, h, n_token, mem_idx, mem_score, tie_flag, stream);
    c.it_begin = it_begin; c.it_end = it_end;
    IPSX_TRY(validate_scan_call(c));
    ScanGate g = {};
    g.wait = gate; g.target = gate_target; g.publish = gate_publish; g.status = status; g.bit = status_bit;
    g.out = reinterpret_cast<long long*>(mem_out);
    g.wait_ticks = (unsigned long long)g_persist_wait_ms * 100000ull;
    return launch_scan_mnist_gate(c, scan_logits_table(logits, parts, n_parts, part_begin, part_end, d, pos, pos_bstride, v_packed, redo, redo_mask), g);
}

IPSX_API int ipsx_set_persistent_wait_ms(int ms) {
    const int prev = g_persist_wait_ms;
    if (ms > 0) g_persist_wait_ms = ms > 20000 ? 20000 : ms;
    return prev;
}

IPSX_API int ipsx_set_tie_order(int mode) {
    const int prev = ipsx::g_tie_order;
    if (mode >= 0 && mode <= 2) ipsx::g_tie_order = mode;
    return prev;
}

// Diagnostic (not part of include/ipsx.h): copies g_persist_log to out8 (host memory) and clears it; synchronises the device
extern "C" __attribute__((visibility("default"))) int ipsx_dbg_persist_log(unsigned long long* out8) {
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(ipsx::g_persist_log), sizeof(zero)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(ipsx::g_persist_log), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}

// Diagnostic entry point (not part of include/ipsx.h): when set to a device buffer of b*8 uint64, the next
// resident scans accumulate per-phase s_memtime cycles there (tools/scan_stamps.py); NULL switches it off.
extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_stamps(unsigned long long* buf) {
    ipsx::g_scan_stamps = buf;
}

// Diagnostic entry point (not part of include/ipsx.h): nonzero sends every shape through the generic loop kernel
// (scan_large_kernel) - tools/scan_compare.py holds the two loop kernels against each other this way.
extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_generic(int on) { g_scan_generic = on != 0; }

extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_direct(int on) { g_scan_direct = on != 0; }
// Diagnostic: workgroups per image for candidate sets beyond the LDS (-1 the default, 0 / 1 one workgroup, 2 / 4 / 8)
extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_team(int w) { g_scan_team = w; }
// Diagnostic: 0 = the team's ranking always from whole runs (the path taken when the runs' top halves are not provably enough)
extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_team_trunc(int on) { g_scan_team_trunc = on != 0; }
// Diagnostic: 0 sends the shape of scan_cam_kernel (8 logits per candidate, M = I = 256) through scan_fast_kernel instead -
// tools/scan_compare.py and tools/scan_stamps.py use it.
extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_r8(int on) { g_scan_r8 = on != 0; }
// Diagnostic: 0 sends the shape of scan_mnist_kernel (8 heads, 4 tokens, M = I = 64) through scan_fast_kernel (tools/scan_compare.py,
// tests/test_scan_mnist.py, the A/B measurements); ipsx_dbg_scan_mnist_shape is the dispatcher's shape predicate
extern "C" __attribute__((visibility("default"))) void ipsx_dbg_scan_mnist(int on) { g_scan_mnist = on != 0; }
// Diagnostic: 0 = ipsx_scan_range_logits enqueues the launches it replaces (logits_kernel<1> per part, the loop's range, the
// conditional redo) instead of the one launch with the logits prologue (tests/test_scan_logits.py, the A/B measurements);
// -1 only queries.  -> the previous setting
extern "C" __attribute__((visibility("default"))) int ipsx_dbg_scan_logits(int on) {
    const int prev = g_scan_logits ? 1 : 0;
    if (on >= 0) g_scan_logits = on != 0;
    return prev;
}
extern "C" __attribute__((visibility("default"))) int ipsx_dbg_scan_mnist_shape(int m, int i, int h, int n_token) {
    return scan_mnist_shape(m, i, h, n_token) ? 1 : 0;
}
