// scan_mnist.hip - scan_mnist_kernel: the LDS-resident selection loop specialised for BASELINE configs[1] / [2]
// (Megapixel-MNIST: 8 heads, 4 query tokens, M = I = 64; reference loop architecture/ips_net.py:213-241, scores
// transformer.py:143-148).

#include <algorithm>
#include <cstdlib>

#include "logits_wave.h"
#include "scan_common.h"

namespace ipsx {

// ---------------------------------------------------------------------------------------------------------------
// scan_mnist_kernel: 32 logits per candidate (row r = head * 4 + token), at most 128 candidates per iteration, one
// workgroup of 1,024 threads per image.  The same arithmetic as scan_fast_kernel, every sum in the contract's order
// (DESIGN 4): bit-identical indices, scores, tie flags and resumed ranges (tools/scan_compare.py, tests/test_scan_mnist.py).
//
// scan_fast_kernel at this shape is a chain of nine barriers around short phases whose every size is a runtime value.
// What this kernel does instead:
//   * every size is a compile-time constant: LDS addresses are immediates, no loop over runtime M / I; the scalar
//     registers the compiler spills to vector lanes (61) are written in the prologue and read back behind the non-inlined
//     tie replay only - an iteration without a tie has no v_readlane / v_writelane and no scratch access;
//   * no transposition of the weights through LDS: thread (candidate l, token t) of waves 0..7 reads the 8 exponentials
//     and the 8 reciprocals of its token (rows of 36 words: conflict-free), multiplies, adds the heads in ascending order,
//     and the 4 tokens of a candidate meet through quad permutes - one phase and one barrier less;
//   * waves 8..15 prepare the next chunk meanwhile (logits, speculative exponentials, row maxima);
//   * ALL 128 candidates are ranked by counting on their 64-bit keys, 8 threads per key with 16 keys each, eight 16-byte
//     reads at immediate offsets: two instructions per comparison, exact under ties - so neither the threshold of the
//     lowest memory score (an LDS minimum, a compaction and two barriers to save eight comparisons per thread) nor
//     32-bit score keys (three instructions per comparison plus the tie test) nor a sorted run of the memory wave pay
//     at 128 candidates; dropped by arithmetic, the first also because ranking everything IS scan_fast_kernel's tie path;
//   * the row maxima live in two sets of key words by parity, so an iteration whose maxima did not move (almost all)
//     goes from the first barrier straight to the row sums;
//   * every wave tests the ranked neighbours for equal scores on its own (two reads and a ballot): without one - the
//     common case - no flag, no barrier; with one, scan_fast_kernel's test of the runs and the replay of torch.topk;
//   * the first iteration of a launch evaluates its 4,096 exponentials on all threads, not column by column.
// Four barriers per iteration instead of nine.
namespace mn {
constexpr int M = 64, I = 64, L = 128, R = 32, H = 8, T = 4, LD = 36, NT = 1024;
constexpr int OFF_KEYA = 0;                          // u64[L]: every candidate's key by position
constexpr int OFF_SORTED = OFF_KEYA + L * 8;         // u64[L]: the ranked keys
constexpr int OFF_CAND = OFF_SORTED + L * 8;         // int[2][L]: patch index of every candidate (two sets)
constexpr int OFF_PMAX = OFF_CAND + 2 * L * 4;       // u32[2][2 R]: row-maximum keys, [memory R | chunk R], by parity
constexpr int OFF_CNT = OFF_PMAX + 4 * R * 4;        // int[8]: [2], [3] replay flag (by parity), [6] rows known
constexpr int OFF_PREV = OFF_CNT + 32;               // u32[2][R]: bits of the previous row maxima, by parity
constexpr int OFF_DEN = OFF_PREV + 2 * R * 4;        // float[R]
constexpr int OFF_X = (OFF_DEN + R * 4 + 15) & ~15;  // float[2][L][LD]: logits
constexpr int OFF_E = OFF_X + 2 * L * LD * 4;        // float[2][L][LD]: exponentials
constexpr int OFF_STK = OFF_E + 2 * L * LD * 4;      // scratch of the tie replay
constexpr int LDS_BYTES = OFF_STK + STK_BYTES;
static_assert(OFF_KEYA % 16 == 0 && OFF_X % 16 == 0 && (LD * 4) % 16 == 0, "16-byte rows");
static_assert(H * T == R && M + I == L && L * 8 == NT, "scan_mnist_kernel: 8 threads per key");
static_assert(OFF_STK == 77728, "scan_mnist_kernel: 77,728 B of LDS + the replay's scratch (STK_BYTES)");
static_assert(LDS_BYTES <= 160 * 1024, "scan_mnist_kernel: LDS");
}  // namespace mn

// the value lane (lane & ~3) + K holds, K a constant: a quad permute
template <int K>
__device__ __forceinline__ float quad_bcast(float v) {
    return as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)as_u32(v), K * 0x55, 0xF, 0xF, false));
}

// PRO: the launch computes its image's logits itself, in a prologue in front of the first iteration of its range.  A patch's
// logits depend on that patch alone, and workgroup b reads image b's logits alone - so workgroup b writes the rows of image b
// that its range adds (the parts [part0, part1) of the call, ScanLogits) into the (b, n, R) table logits_kernel<1> fills
// otherwise, with logits_wave's arithmetic (the 32-row tiles of a part dealt to the 16 wavefronts; four k-groups of loads in
// flight instead of eight: 128 registers), and a barrier with a workgroup-scope release / acquire around it hands them to
// the loop: no logits launch in front of the loop's, no dependency between workgroups, no wait.  With the word `redo` set
// (a part wait of the call gave up: rows may have been computed from embeddings that were not there yet) it computes ALL
// parts and runs the loop from iteration 0 - what three conditional logits launches and a conditional loop launch did.
// The arguments of the prologue are a second kernel parameter that only a PRO instantiation has (P...): the others keep
// their one-parameter shape and their code (tools/asm_compare.py; PRO in front keeps the order of their mangled names).
//
// GATE (a third parameter, ScanGate, behind the prologue's): the two ends of a hand-over between two launches of one call
// that lie on different streams with no stream wait between them (Selection.parts_loop_logits).
//   publish  the launch in front - the side stream's last - stores the iteration it reached, it1, to publish[b] at its very
//            end, behind its workgroup's stores of mem_idx / mem_score / tie: parts_count's hand-over (fused_trunk_eight.h).
//   wait     the launch behind - the call's last, enqueued on the main stream directly behind the trunk - writes its parts'
//            rows FIRST, beside the other launch's last iterations, and only then polls wait[b] until it has reached `target`
//            (relaxed agent-scope loads, a sleep between them, one agent-scope acquire behind the barrier that tells the
//            workgroup): stream order makes the one word per image enough - when the side's last launch has ended for image
//            b, every earlier side-stream kernel of the call has ended.  A wait that sees no progress of its word for
//            wait_ticks gives up: it sets `bit` in *status, as a part wait does, and does what `redo` makes it do - every
//            part's rows, the loop from iteration 0.
//   out      the final memory indices go here instead of mem_idx: a launch that gave up may still have a late side-stream
//            launch writing the working buffer behind it.
// Without the prologue (scan_mnist_kernel<false, false, ScanGate>) the parameter is the kernel's second and only `publish` is
// looked at: the side stream's last loop launch behind a long part's logits launch, at the plain instance's registers.
// With `redo` set on entry the wait comes FIRST (still bounded): the rows a side-stream launch wrote from embeddings that
// were not there yet must not land behind the ones this launch writes.  (A part wait cannot give up after the trunk's end -
// its counter is full by then, and a wait that starts later passes at once - so the word this launch reads at its start,
// behind the trunk in stream order, is final as far as part waits go.)
// The wait side of ScanGate (see scan_mnist_kernel), by the whole workgroup: wave 0 polls wait[b] until it has reached the target -
// part_wait_kernel's form: relaxed agent-scope loads, a sleep between them, bounded WITHOUT PROGRESS of the word -, a barrier
// tells the others, ONE agent-scope acquire orders every wave's loads behind the poll.  -> reached (workgroup-uniform, scalar).
__device__ __forceinline__ bool gate_reached(const ScanGate& g, int b, int* flag) {
    if (threadIdx.x < 64) {
        unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        int last = __hip_atomic_load(g.wait + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 1;
        while (last < g.target) {
            __builtin_amdgcn_s_sleep(8);
            const int v = __hip_atomic_load(g.wait + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long t = __builtin_amdgcn_s_memrealtime();
            if (v != last) { last = v; t0 = t; }
            else if (t - t0 > g.wait_ticks) { ok = 0; break; }
        }
        if (threadIdx.x == 0) *flag = ok;
    }
    lds_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int ok = __builtin_amdgcn_readfirstlane(*flag);
    lds_barrier();                                               // (the flag is read before anybody writes it again)
    return ok != 0;
}

template <typename A, typename... B>
__device__ __forceinline__ const A& first_of(const A& a0, const B&...) { return a0; }

template <typename A>
__device__ __forceinline__ const A& last_of(const A& a0) { return a0; }
template <typename A, typename... B>
__device__ __forceinline__ const auto& last_of(const A&, const B&... rest) { return last_of(rest...); }

template <bool PRO, bool PERSIST, typename... P>
__global__ __launch_bounds__(mn::NT) void scan_mnist_kernel(ScanArgs a, P... p) {
    using namespace mn;
    constexpr bool GATE = sizeof...(P) == (PRO ? 2 : 1);        // (without the prologue: a launch that publishes, and nothing else)
    static_assert((sizeof...(P) == (PRO ? 1 : 0) || GATE) && !((PRO || GATE) && PERSIST),
                  "scan_mnist_kernel: the prologue's arguments (and the gate's behind them), plain launches only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (!PERSIST && scan_skipped(a.cond, a.cond_mask)) return;
    if constexpr (PRO) {
        const ScanLogits& q = first_of(p...);
        int k0 = q.part0, k1 = q.part1;
        // (the word is the same for every lane: through readfirstlane, so that it0 and everything the iterations derive from it
        //  stay in scalar registers as in the other instantiations)
        int redo = 0;
        if (q.redo != nullptr)
            redo = __builtin_amdgcn_readfirstlane(__hip_atomic_load(q.redo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & q.redo_mask);
        if (redo != 0) { k0 = 0; k1 = q.n_parts; a.it0 = 0; }
        int s0 = 0, s1 = 0;                                       // GATE: the parts whose rows are written already (second pass)
        if constexpr (GATE) {
            const ScanGate& g = last_of(p...);
            if (g.wait != nullptr && redo != 0 && !gate_reached(g, (int)blockIdx.x, reinterpret_cast<int*>(smem + OFF_CNT)) && threadIdx.x == 0)
                __hip_atomic_fetch_or(g.status, g.bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (;;) {                                                // (GATE: a second pass when the wait gave up)
#pragma unroll 1
            for (int k = k0; k < k1; ++k) {
                if (GATE && k >= s0 && k < s1) continue;
                LogitsArgs la;                                    // part k: (b, rows, d) embeddings of the rows first .. first + rows
                la.emb = q.part[k].emb; la.emb_bs = (long long)q.part[k].rows * q.d;
                la.pos = q.pos ? q.pos + (size_t)q.part[k].first * q.d : nullptr; la.pos_bs = q.pos_bs;
                la.vp = q.vp; la.n = q.part[k].rows; la.d = q.d; la.R = R; la.kgs = q.kgs;
                la.out = q.out + (size_t)q.part[k].first * R; la.out_bs = a.n * R;
                if (q.pos) {                                      // (workgroup-uniform, known in front of the loads)
                    for (unsigned bx = 0; (long long)bx * (NT / 2) < la.n; ++bx) logits_wave<1, 4, NT / 64, 1>(la, bx, (int)blockIdx.x);
                } else {
                    for (unsigned bx = 0; (long long)bx * (NT / 2) < la.n; ++bx) logits_wave<1, 4, NT / 64, -1>(la, bx, (int)blockIdx.x);
                }
            }
            if constexpr (GATE) {
                const ScanGate& g = last_of(p...);
                if (g.wait != nullptr && redo == 0 && !gate_reached(g, (int)blockIdx.x, reinterpret_cast<int*>(smem + OFF_CNT))) {
                    // gave up: the redo, in this workgroup alone (workgroup-uniform): the other parts' rows, the loop from 0
                    if (threadIdx.x == 0) __hip_atomic_fetch_or(g.status, g.bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    redo = 1; s0 = k0; s1 = k1; k0 = 0; k1 = q.n_parts; a.it0 = 0;
                    continue;
                }
            }
            break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // every row is written before the barrier below ...
    }
    __builtin_amdgcn_s_setprio(3);
    if (PERSIST) {
        asm volatile("v_mov_b32 v127, 0" ::: "v127");               // (the whole register file of the compute unit: see scan_fast_kernel)
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_or(a.status, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.plog[4], (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    uint64_t* const keyA = reinterpret_cast<uint64_t*>(smem + OFF_KEYA);
    uint64_t* const sorted = reinterpret_cast<uint64_t*>(smem + OFF_SORTED);
    uint32_t* const pmax = reinterpret_cast<uint32_t*>(smem + OFF_PMAX);
    int* const ccount = reinterpret_cast<int*>(smem + OFF_CNT);
    uint32_t* const prevk = reinterpret_cast<uint32_t*>(smem + OFF_PREV);
    float* const rden = reinterpret_cast<float*>(smem + OFF_DEN);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r = tid & (R - 1);
    const int hid = tid - 512;                                  // helper index (waves 8..15), < 0 on the key waves
    const float* const lg = a.lg + (size_t)b * a.n * R;
    int ready_known = 0;
    if (tid < 4 * R) pmax[tid] = 0u;
    if (tid < 2) ccount[2 + tid] = 0;
    lds_barrier();
    if constexpr (PRO) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");      // ... and read behind it
    SCAN_WAIT_ROWS(std::min<long long>(a.n, a.it0 * (long long)I + M + I));
    {
        float* const x0 = reinterpret_cast<float*>(smem + OFF_X);
        int* const cand0 = reinterpret_cast<int*>(smem + OFF_CAND);
        uint32_t km = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {                            // memory rows: 2,048 logits, two per thread
            const int l = (tid >> 5) + 32 * k;
            const size_t row = a.it0 == 0 ? (size_t)l : (size_t)a.mem_idx[(size_t)b * M + l];
            const float v = scan_load<PERSIST>(lg + row * R + r);
            x0[l * LD + r] = v;
            km = max(km, max_key(v));
        }
        fold_row_max<R>(km, pmax, lane);                        // set 0: read by the first iteration
        if (tid < M) cand0[tid] = a.it0 == 0 ? tid : (int)a.mem_idx[(size_t)b * M + tid];
    }
    const long long n_iter = a.it1 - a.it0;
    float pf[4];
    {
        float* const x0 = reinterpret_cast<float*>(smem + OFF_X);
        int* const cand0 = reinterpret_cast<int*>(smem + OFF_CAND);
        const long long lo = a.it0 * (long long)I + M;
        const int cnt = n_iter > 0 ? (int)std::min<long long>(I, a.n - lo) : 0;
        uint32_t kc = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {                            // first chunk: straight into its rows
            const int e = tid + NT * k;
            if (e < cnt * R) {
                const float v = scan_load<PERSIST>(lg + (size_t)lo * R + e);
                x0[(M + (e >> 5)) * LD + r] = v;
                kc = max(kc, max_key(v));
            }
        }
        fold_row_max<R>(kc, pmax + R, lane);
        if (tid < cnt) cand0[M + tid] = (int)(lo + tid);
        const long long lo1 = lo + I;
        const int cnt1 = n_iter > 1 ? (int)std::max<long long>(0, std::min<long long>(I, a.n - lo1)) : 0;
        if (cnt1 > 0) SCAN_WAIT_ROWS(lo1 + cnt1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = hid + 512 * k;
            pf[k] = (hid >= 0 && e < cnt1 * R) ? scan_load<PERSIST>(lg + (size_t)lo1 * R + e) : 0.0f;
        }
    }
    int tie = 0;
    const int n_it = (int)n_iter, n_rows = (int)a.n;             // (n < 2^31: 32-bit row arithmetic inside the loop)
    for (int k_it = 0; k_it < n_it; ++k_it) {
        const int lo = ((int)a.it0 + k_it) * I + M;
        const int cnt = min(I, n_rows - lo);
        const int Lc = M + cnt;                                  // candidates of this iteration (128 but for a ragged last chunk)
        const int par = k_it & 1;
        // current / spare buffers by parity; everything else sits at a fixed address
        float* const xc = reinterpret_cast<float*>(smem + OFF_X) + par * (L * LD);
        float* const xn = reinterpret_cast<float*>(smem + OFF_X) + (par ^ 1) * (L * LD);
        float* const ec = reinterpret_cast<float*>(smem + OFF_E) + par * (L * LD);
        float* const en = reinterpret_cast<float*>(smem + OFF_E) + (par ^ 1) * (L * LD);
        int* const cand = reinterpret_cast<int*>(smem + OFF_CAND) + par * L;
        int* const cnew = reinterpret_cast<int*>(smem + OFF_CAND) + (par ^ 1) * L;
        uint32_t* const mkey = pmax + 2 * R * par;              // row-maximum keys read by this iteration: [memory | chunk]
        uint32_t* const mkey_nx = pmax + 2 * R * (par ^ 1);     // ... and folded into by this iteration, for the next one
        const int lo1 = lo + I;
        const int cnt1 = k_it + 1 < n_it ? max(0, min(I, n_rows - lo1)) : 0;
        lds_barrier();                                          // B0: this iteration's rows, maxima and candidates are in place
        // P1: row maxima from the two key words of the row; exp(x - max) wherever a maximum moved
        if (tid == 0) ccount[2 + (par ^ 1)] = 0;
        const uint32_t mbits = as_u32(max_key_value(max(mkey[r], mkey[R + r])));
        const float rowmax = as_float(mbits);
        const bool changed = k_it == 0 || prevk[par * R + r] != mbits;
        if (tid < R) prevk[(par ^ 1) * R + r] = mbits;
        {
            unsigned long long moved = __ballot(changed) & 0xFFFFFFFFull;       // lane r < R holds row r: the same on every wave
            if (moved != 0ull) {
                if (__popcll(moved) >= 8) {
                    // many rows (the first iteration of a launch: all of them): an element per thread, four rounds
                    if (changed) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int l = (tid >> 5) + 32 * k;
                            if (l < Lc) ec[l * LD + r] = det_expf_np(xc[l * LD + r] - rowmax);
                        }
                    }
                } else {
                    // a column of Lc elements, one per thread of the first two waves
                    while (moved) {
                        const int rr = __ffsll((long long)moved) - 1;
                        moved &= moved - 1ull;
                        exp_column(xc + rr, ec + rr, Lc, LD, __shfl(rowmax, rr, 64));
                    }
                }
                lds_barrier();                                  // B1 (workgroup-uniform: only when exponentials were rewritten)
            }
        }
        // P3: softmax denominators in the contract's order (lane j adds candidates j, j + 64, then the xor butterfly), rows
        // wave and wave + 16
        {
            const float* const col = ec + lane * LD + wave;
            const float a0 = col[0], a1 = col[64 * LD], b0 = col[16], b1 = col[64 * LD + 16];      // (rows beyond Lc: stale, masked)
            const bool has1 = lane + 64 < Lc;                    // (lane < 64 < Lc always)
            float s0 = 0.0f, s1 = 0.0f;
            s0 = s0 + a0; s1 = s1 + b0;
            s0 = s0 + (has1 ? a1 : 0.0f); s1 = s1 + (has1 ? b1 : 0.0f);
            wave_sum2(s0, s1, lane);
            if (lane == 0) { rden[wave] = 1.0f / s0; rden[wave + 16] = 1.0f / s1; }       // (reciprocals: one division per row)
        }
        lds_barrier();                                          // B2: everybody has read the maxima, the reciprocals are in place
        if (tid < 2 * R) mkey[tid] = 0u;                        // cleared for the folds of the NEXT iteration (into this set)
        if (wave < 8) {
            // P4: thread (candidate l, token t): weights e * (1 / den) of its 8 heads added in ascending order, mean over the
            // heads; then the 4 tokens of the candidate in ascending order, mean over the tokens - the operations of
            // scan_fast_kernel's weight and score phases
            const int l = tid >> 2, t = tid & 3;
            const float* const er = ec + l * LD + t;
            float ev[H], dn[H];
#pragma unroll
            for (int hh = 0; hh < H; ++hh) { ev[hh] = er[hh * T]; dn[hh] = rden[hh * T + t]; }
            float sh = 0.0f;
#pragma unroll
            for (int hh = 0; hh < H; ++hh) sh = sh + ev[hh] * dn[hh];
            const float q = l < Lc ? sh / (float)H : 0.0f;
            float st = 0.0f;
            st = st + quad_bcast<0>(q); st = st + quad_bcast<1>(q); st = st + quad_bcast<2>(q); st = st + quad_bcast<3>(q);
            if (t == 0) keyA[l] = l < Lc ? rank_key(st / (float)T, (uint32_t)l) : 0ull;     // (no candidate: 0 sorts last)
        } else {
            // prep of the next chunk into the SPARE buffers: its logits, its exponentials under this iteration's maxima (right
            // unless a maximum moves - checked bitwise by the next iteration), its share of the chunk rows' maxima
            uint32_t kc = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = (hid >> 5) + 16 * k;
                if (row < cnt1) {
                    xn[(M + row) * LD + r] = pf[k];
                    en[(M + row) * LD + r] = det_expf_np(pf[k] - rowmax);
                    kc = max(kc, max_key(pf[k]));
                }
            }
            fold_row_max<R>(kc, mkey_nx + R, lane);
            if (hid < cnt1) cnew[M + hid] = (int)(lo1 + hid);
        }
        lds_barrier();                                          // B3: every key is in place
        {
            // P5: rank = number of larger keys.  Thread (key kk, part p) counts keys 2 p + 16 i and 2 p + 16 i + 1, i < 8; the 8
            // parts of a key meet by an xor butterfly (integer adds); part 0 places the key
            const int kk = tid >> 3, p = tid & 7;
            const uint64_t mine = keyA[kk];
            const ulonglong2* const kp = reinterpret_cast<const ulonglong2*>(keyA) + p;
            ulonglong2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = kp[8 * i];
            uint32_t c = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) c += (v[i].x > mine ? 1u : 0u) + (v[i].y > mine ? 1u : 0u);
            c += lane_xor_u32<1>(c, lane);
            c += lane_xor_u32<2>(c, lane);
            c += lane_xor_u32<4>(c, lane);
            if (p == 0 && mine != 0ull) sorted[c] = mine;
        }
        lds_barrier();                                          // B4: the ranking is in place
        {
            // equal scores among the first M + 1 ranks (Lc > M: ranks 0 .. M exist)?  Every wave looks for itself - the same
            // data, the same answer, no flag and no barrier in the common case
            const uint32_t* const sw = reinterpret_cast<const uint32_t*>(sorted);
            const unsigned long long eqm = __ballot(sw[2 * lane + 1] == sw[2 * lane + 3]);
            if (eqm != 0ull) {
                // scan_fast_kernel's test: two candidates of one run of equal scores whose logit rows are bit-identical
                // (tie_order 2: any two of equal score) call for torch.topk's order.  A run that reaches the first M + 1 ranks
                // has the score of a winner, so all of it is ranked wherever scan_fast_kernel's threshold would have cut.
                if (a.tie_order != 0) {
                    bool hit = false;
                    for (int j = tid; j < M && !hit; j += NT)
                        for (int k = j + 1; k < Lc && !hit && (sorted[k] >> 32) == (sorted[j] >> 32); ++k) {
                            bool same = true;
                            if (a.tie_order == 1) {
                                // (every read issued before the compare, no short circuit: 32 nested lane masks were 60 spilled
                                //  scalar registers)
                                const uint4* ra = reinterpret_cast<const uint4*>(xc + key_pos(sorted[j]) * LD);
                                const uint4* rb = reinterpret_cast<const uint4*>(xc + key_pos(sorted[k]) * LD);
                                uint32_t diff = 0u;
#pragma unroll
                                for (int rr = 0; rr < R / 4; ++rr) {
                                    const uint4 va = ra[rr], vb = rb[rr];
                                    diff |= (va.x ^ vb.x) | (va.y ^ vb.y) | (va.z ^ vb.z) | (va.w ^ vb.w);
                                }
                                same = diff == 0u;
                            }
                            hit = hit || same;
                        }
                    if (__ballot(hit) != 0ull && lane == 0) ccount[2 + par] = 1;
                }
                lds_barrier();
                if (tid == 0 && (eqm >> (M - 1)) != 0ull) tie = 1;       // ranks M - 1 and M: bit-equal score keys (two NaNs tie)
                if (a.tie_order != 0 && ccount[2 + par] != 0)
                    tie_order_slow(sorted, keyA, Lc, M, reinterpret_cast<int*>(smem + OFF_STK));
            }
        }
        {
            // the loads of the chunk after the next one (see scan_fast_kernel): in flight through the gather and the next
            // iteration's first phases
            const int lo2 = lo + 2 * I;
            const int cnt2 = k_it + 2 < n_it ? max(0, min(I, n_rows - lo2)) : 0;
            if (cnt2 > 0) SCAN_WAIT_ROWS(lo2 + cnt2);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = hid + 512 * k;
                pf[k] = (hid >= 0 && e < cnt2 * R) ? scan_load<PERSIST>(lg + (size_t)lo2 * R + e) : 0.0f;
            }
        }
        // P6: new memory into the other buffers.  Waves 0..7: the logit rows, four elements per thread (rows (tid >> 5) + 16 k,
        // column r), and the new rows' maxima; waves 8..15: the exponentials, 16 bytes per thread, and the patch indices.
        {
            const uint32_t* const spos = reinterpret_cast<const uint32_t*>(sorted);         // word 2 j: ~position of rank j
            if (wave < 8) {
                uint32_t p[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) p[k] = ~spos[2 * ((tid >> 5) + 16 * k)] & (L - 1);
                float gx[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) gx[k] = xc[p[k] * LD + r];
                uint32_t km = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) { xn[((tid >> 5) + 16 * k) * LD + r] = gx[k]; km = max(km, max_key(gx[k])); }
                fold_row_max<R>(km, mkey_nx, lane);                // maxima of the NEW memory rows, for the next iteration
            } else {
                const int j = hid >> 3, qd = (hid & 7) * 4;
                const uint32_t p = ~spos[2 * j] & (L - 1);
                const uint32_t pc = ~spos[2 * (hid & (M - 1))] & (L - 1);
                const float4 ge = *reinterpret_cast<const float4*>(ec + p * LD + qd);
                const int ci = cand[pc];
                *reinterpret_cast<float4*>(en + j * LD + qd) = ge;
                if (hid < M) cnew[hid] = ci;
            }
        }
        // no barrier here: B0 of the next iteration orders the gather before anybody reads the new buffers
    }
    lds_barrier();
    {
        const int parn = (int)(n_iter & 1);                       // the set the last iteration wrote
        const int* const cand = reinterpret_cast<const int*>(smem + OFF_CAND) + parn * L;
        long long* dst = a.mem_idx;
        if constexpr (GATE) {
            const ScanGate& g = last_of(p...);
            if (g.out != nullptr) dst = g.out;
        }
        if (tid < M) {
            dst[(size_t)b * M + tid] = cand[tid];
            if (a.mem_score) a.mem_score[(size_t)b * M + tid] = n_iter > 0 ? key_score(sorted[tid]) : 0.0f;
        }
    }
    if (a.tie && tid == 0 && tie) a.tie[b] = 1;
    if constexpr (GATE) {
        const ScanGate& g = last_of(p...);
        if (g.publish != nullptr) {
            // parts_count's hand-over: the storing wavefronts drain their stores, the workgroup meets, one thread releases at
            // agent scope, waits for the write-back, and only then stores the word
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(g.publish + b, (int)a.it1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

bool scan_mnist_shape(int m, int i, int h, int n_token) { return h == mn::H && n_token == mn::T && m == mn::M && i == mn::I; }

int launch_scan_mnist(const ScanCall& c) {
    IPSX_REQUIRE(scan_mnist_shape(c.m, c.i, c.h, c.n_token) && c.rows == Rows::Packed && (c.workgroups <= 0 || c.workgroups >= c.b),
                 "scan_mnist_kernel: 8 heads x 4 tokens, M = I = 64, contiguous logits, one workgroup per image");
    ScanArgs a;
    fill_scan_args(a, c);
    a.stk_off = mn::OFF_STK;
    launch_lds(c.ready ? scan_mnist_kernel<false, true> : scan_mnist_kernel<false, false>, dim3((unsigned)c.b), dim3(mn::NT), mn::LDS_BYTES,
               c.stream, a);
    return launched("scan");
}

// the loop's range with the logits prologue (scorer.hip has checked the part table: ipsx_scan_logits_check)
int launch_scan_mnist_logits(const ScanCall& c, const ScanLogits& p) {
    IPSX_REQUIRE(scan_mnist_shape(c.m, c.i, c.h, c.n_token) && c.rows == Rows::Packed && !c.ready && !c.cond && c.workgroups <= 0,
                 "scan_mnist_kernel with logits: 8 heads x 4 tokens, M = I = 64, packed logits, a plain launch of one workgroup per image");
    ScanArgs a;
    fill_scan_args(a, c);
    a.stk_off = mn::OFF_STK;
    launch_lds(scan_mnist_kernel<true, false, ScanLogits>, dim3((unsigned)c.b), dim3(mn::NT), mn::LDS_BYTES, c.stream, a, p);
    return launched("scan_logits");
}

// ... and with the gate's arguments (scorer.hip: ipsx_scan_range_logits_gate has checked them)
int launch_scan_mnist_gate(const ScanCall& c, const ScanLogits& p, const ScanGate& g) {
    IPSX_REQUIRE(scan_mnist_shape(c.m, c.i, c.h, c.n_token) && c.rows == Rows::Packed && !c.ready && !c.cond && c.workgroups <= 0,
                 "scan_mnist_kernel with logits: 8 heads x 4 tokens, M = I = 64, packed logits, a plain launch of one workgroup per image");
    ScanArgs a;
    fill_scan_args(a, c);
    a.stk_off = mn::OFF_STK;
    // a launch that only publishes - no rows of its own, no redo, no wait, no buffer of its own: the side stream's last loop launch
    // behind a long part's logits launch - is the plain instance with the gate's parameter: none of the prologue's registers
    // (tools/scan_loop_time.py: the loop alone at the plain instance's time per iteration)
    if (p.part0 == p.part1 && !p.redo && !g.wait && !g.out)
        launch_lds(scan_mnist_kernel<false, false, ScanGate>, dim3((unsigned)c.b), dim3(mn::NT), mn::LDS_BYTES, c.stream, a, g);
    else
        launch_lds(scan_mnist_kernel<true, false, ScanLogits, ScanGate>, dim3((unsigned)c.b), dim3(mn::NT), mn::LDS_BYTES, c.stream, a, p, g);
    return launched("scan_logits_gate");
}

}  // namespace ipsx
