// Row-parallel fused hidden stack (reference: /root/reference/locator/locator.py:319-325, :314-315).
//
// The rows of a minibatch are independent through every Dense+ELU layer, the Dropout, the two
// Dense(2) heads and the per-sample Euclidean loss; only the weight gradients reduce over rows.  So
// instead of one launch per layer (latency-bound: ~5 us each, 20 per step), ONE launch carries each
// group of R batch rows through all layers forward, the heads and the loss, and all layers
// backward, with no communication between workgroups at all.  Every workgroup streams each layer's
// 256 KB kernel from L2 (coalesced 16-byte loads; the backward pass reads a transposed copy kept in
// sync by the Adam kernel), contracting on the vector ALU (R rows is far below an MFMA tile).  The
// stream is a register ring of untracked asm loads with hand-counted waits (round 7): a slot of rows is
// requested again the moment it has been consumed, across layer boundaries, so that a layer's worth of
// requests stays in flight through the reduction, the barriers and the epilogue of every pass; the
// compiler's own counting put a full drain in front of every backward pass.  The
// row-reducing work — dW, db and Adam for all hidden layers and the heads, and the batch loss — runs
// afterwards in ONE wide launch (stack_dw_all_kernel), one workgroup per 32x32 weight tile.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "step_args.h"

#ifndef SF_THREADS
#define SF_THREADS 512
#endif

// The weight ring and every other load of a worker are untracked loads with hand-counted waits (gload16_uniform,
// gload4_inout, gload1_inout, vm_wait, vm_wait_slot, vm_landed: common.h, with the counting rule).  The workgroup barrier is
// lds_barrier(): inside stack_fused_kernel no thread ever reads another thread's GLOBAL writes, and __syncthreads() would
// drain the ring.

// e0^2 + e1^2 of the loss, with its roundings written out.  Left to the compiler, which product is fused into the sum is its
// choice per instantiation, and it changes with unrelated code around it (a distance then moves by an ulp and val_loss with it).
// These are the forms the kernels have had since round 1: the training launch rounds both products and adds them, the eval
// launch rounds e0^2 and fuses e1^2 into the sum.
__device__ __forceinline__ float sf_sumsq_train(float e0, float e1) {
#pragma clang fp contract(off)
    const float a = e0 * e0, b = e1 * e1;
    return b + a;
}
__device__ __forceinline__ float sf_sumsq_eval(float e0, float e1) { return fmaf(e1, e1, e0 * e0); }

template <int NHT, int R, bool TRAIN>
__global__ __launch_bounds__(SF_THREADS) void stack_fused_kernel(
    const float* __restrict__ a1_in, const float* __restrict__ Wh, const float* __restrict__ WhT,
    const float* __restrict__ bh, const float* __restrict__ wa, const float* __restrict__ ba,
    const float* __restrict__ wb, const float* __restrict__ bb, const uint8_t* __restrict__ mask, float keep_scale,
    int L, int n_pre, int n_b, const int32_t* __restrict__ rows, const float* __restrict__ Y,
    float* __restrict__ acts, float* __restrict__ adrop, float* __restrict__ dz, float* __restrict__ head_out,
    float* __restrict__ yhat, float* __restrict__ dist, int xcd_stride, int n_work, int slot_rows,
    const float* __restrict__ rd_partial, int rd_G, int64_t rd_MH, const float* __restrict__ rd_cvec8,
    const float* __restrict__ rd_b1) {
    constexpr int Hp = NHT * 32;
    constexpr int C4 = Hp / 4;               // float4 columns per weight row
    constexpr int KG = SF_THREADS / C4;      // k-groups
    constexpr int KPG = Hp / KG;             // k per group
    static_assert(SF_THREADS % C4 == 0 && Hp % KG == 0 && KPG >= 1, "unsupported width for the fused stack");
    __shared__ __attribute__((aligned(16))) float act[R][Hp];          // current layer input (rows of this block)
    __shared__ __attribute__((aligned(16))) float part[KG][R][Hp];     // per-k-group partial sums
    __shared__ float hs[R][8];

    // xcd_stride > 1: only every xcd_stride-th workgroup works, so (with the observed block -> XCD b % 8
    // dispatch) all row groups share ONE XCD's L2 and each weight line crosses the fabric once.  Pure
    // speed hint: results do not depend on where workgroups land.
    if (xcd_stride > 1 && (blockIdx.x % xcd_stride) != 0) return;
    const int li = xcd_stride > 1 ? blockIdx.x / xcd_stride : blockIdx.x;      // logical workgroup index
    if (li >= n_work) {
        // L2 warm-up helper (same XCD as the workers under the observed block -> XCD dispatch): touch every
        // weight line in pass order so the workers' loads hit this XCD's L2 (~110 GB/s per CU) instead of
        // waiting on the fabric (~65 GB/s per CU).  Results cannot depend on it: the values are discarded.
        // with stride 8/n_x the logical workgroups cycle over n_x XCDs: the helpers that share this one's XCD
        // (every n_x-th) split the weight lines between them, so each XCD's L2 sees all of them
        const int n_x = xcd_stride > 1 ? 8 / xcd_stride : 1;
        const int nh_all = (int)(gridDim.x / (xcd_stride > 1 ? xcd_stride : 1)) - n_work;
        const int hid = (li - n_work) / n_x, nh = nh_all / n_x > 0 ? nh_all / n_x : 1;
        const int64_t n4 = (int64_t)(L - 1) * Hp * Hp / 4;
        const f32x4* w4 = reinterpret_cast<const f32x4*>(Wh);
        f32x4 sink = {0.f, 0.f, 0.f, 0.f};
        for (int64_t i = (int64_t)hid * SF_THREADS + threadIdx.x; i < n4; i += (int64_t)nh * SF_THREADS) {
            f32x4 v = w4[i];
            sink[0] += v[0];
        }
        if (TRAIN && WhT != nullptr) {
            const f32x4* t4 = reinterpret_cast<const f32x4*>(WhT);
            for (int64_t i = n4 - 1 - ((int64_t)hid * SF_THREADS + threadIdx.x); i >= 0; i -= (int64_t)nh * SF_THREADS) {
                f32x4 v = t4[i];                      // backward passes walk the layers from last to first
                sink[1] += v[0];
            }
        }
        asm volatile("" ::"v"(sink[0]), "v"(sink[1]));
        return;
    }
    const int t = threadIdx.x, c4 = t % C4, kq = t / C4;
    const int r0 = li * R;
    const int64_t blk = (int64_t)slot_rows * Hp, HH = (int64_t)Hp * Hp;      // slot = activations of one layer

    // out[r][n] = sum_k in[r][k] * Wcur[k][n]: partial over this thread's k-group, reduced over groups later.
    // The weight stream runs through a register ring: RING rows of the thread's k-group (32 f32x4 at widths 256 and 512, the
    // whole k-group below that) cut into NS slots of RW rows.  A slot is requested again the moment its rows have been
    // consumed, for the chunk one ring length ahead; past the end of a layer that is the NEXT pass's kernel.  So a ring's
    // worth of rows (a whole layer per workgroup up to width 256, 256 KB at width 512) is in flight at all times, across the
    // reduction, the barriers and the epilogue too.  A pass is KPG / RW chunks = a whole number of trips round the ring:
    // every pass starts at slot 0 and the registers are indexed statically while L stays a run-time value.  Every thread
    // still adds its k ascending, so the sums are what they were.
    //
    // From the first ring request to the last epilogue every load of a worker is an untracked asm load and every wait is
    // counted by hand (the rule is above vm_wait): a load the compiler tracks would be waited for with the ring's younger
    // requests, i.e. by draining the ring.  Stores stay plain: nothing waits for them.
    constexpr int RING = KPG < 32 ? KPG : 32;
    constexpr int RW = RING >= 16 ? RING / 8 : 1;      // rows per slot: 4 at widths 256 / 512, 1 at 128 (8 slots) and 64 (2)
    constexpr int NS = RING / RW, NTRIP = KPG / RING;
    constexpr int ROWB = C4 * 16;                      // bytes of a weight row
    static_assert(KPG >= 2 && NS >= 2 && NS * RW == RING && NTRIP * RING == KPG, "a pass must be whole trips round the ring");
    static_assert(ROWB <= 4096 && (RW == 1 || 4096 % ROWB == 0), "row offsets are split into a register part and an immediate");
    // per-thread output slots of the epilogues: element i = t + SF_THREADS*o of the R x Hp block.  Threads past the block
    // (R * Hp < SF_THREADS) request element i % (R * Hp) and drop it: the loads that a wait counts are never conditional.
    constexpr int NO = (R * Hp + SF_THREADS - 1) / SF_THREADS;
    static_assert((R * Hp) % SF_THREADS == 0 || R * Hp < SF_THREADS, "epilogue slots");
    f32x4 ring[RING];
    // a request is (uniform matrix + chunk) + (the thread's own 32-bit byte offset, < 4 * Hp * Hp) + (row in the slot).
    // The instruction's immediate reaches 4095 bytes; rows of a slot beyond that use the offset register + 4096 * n.
    constexpr int NOFF = (RW * ROWB + 4095) / 4096;
    uint32_t toff[NOFF];
#pragma unroll
    for (int n = 0; n < NOFF; ++n) toff[n] = ((uint32_t)(kq * KPG) * C4 + c4) * 16u + 4096u * n;
    auto load_slot = [&](const float* __restrict__ Wsrc, int c, int s) {
        const char* base = reinterpret_cast<const char*>(Wsrc) + (size_t)c * (RW * ROWB);
        static_assert(RW == 1 || RW == 4, "rows per slot");
        gload16_uniform<0>(ring[s * RW], base, toff[0]);
        if constexpr (RW == 4) {
            gload16_uniform<ROWB % 4096>(ring[s * RW + 1], base, toff[ROWB / 4096]);
            gload16_uniform<(2 * ROWB) % 4096>(ring[s * RW + 2], base, toff[2 * ROWB / 4096]);
            gload16_uniform<(3 * ROWB) % 4096>(ring[s * RW + 3], base, toff[3 * ROWB / 4096]);
        }
    };
    auto fma_slot = [&](int c, int s, f32x4 (&acc)[R]) {
#pragma unroll
        for (int j = 0; j < RW; ++j) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float a = act[r][kq * KPG + c * RW + j];
                acc[r][0] = fmaf(a, ring[s * RW + j][0], acc[r][0]);
                acc[r][1] = fmaf(a, ring[s * RW + j][1], acc[r][1]);
                acc[r][2] = fmaf(a, ring[s * RW + j][2], acc[r][2]);
                acc[r][3] = fmaf(a, ring[s * RW + j][3], acc[r][3]);
            }
        }
    };
    // One trip round the ring: chunks c0 .. c0 + NS - 1 of the matrix in the ring are consumed and slot s is requested
    // again for chunk cn + s of Wn, never behind a condition: a register with one chain of definitions stays one register,
    // while a conditional request would have the compiler copy ring registers whose loads are still in flight.  The wait in front of slot s: it was requested one trip ago, and younger than
    // it are the NS - 1 other slots (RW loads each) and, in the LAST trip of a pass, the pass's NO epilogue operands, which
    // are requested right in front of that trip (younger loads that only some waves issue are not counted: they make the
    // wait longer, never shorter).
    auto trip = [&](auto last, int c0, const float* __restrict__ Wn, int cn, f32x4 (&acc)[R]) {
        constexpr int N = (NS - 1) * RW + (decltype(last)::value ? NO : 0);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if constexpr (RW == 4) vm_wait_slot<N>(ring[s * RW], ring[s * RW + 1], ring[s * RW + 2], ring[s * RW + 3]);
            else vm_wait_slot<N>(ring[s * RW]);
            fma_slot(c0 + s, s, acc);
            // the slot's last use comes before its request: the sums pass through an asm statement in front of it, or the
            // compiler would let the FMAs trail the request and keep the old rows in a copy taken before they landed
#pragma unroll
            for (int r = 0; r < R; ++r) vm_landed(acc[r]);
            load_slot(Wn, cn + s, s);
        }
    };
    // On entry the first RING rows of Wcur's k-group are in the ring (or in flight).  `operands` requests the epilogue's
    // operands in front of the last trip, so that exactly RING loads are younger than they are.  The last trip refills the
    // ring from the next pass's kernel; Wnext is always a valid matrix (see wseq).
    auto contract = [&](const float* __restrict__ Wcur, const float* __restrict__ Wnext, auto operands) {
        f32x4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int tr = 0; tr + 1 < NTRIP; ++tr) trip(std::false_type{}, tr * NS, Wcur, (tr + 1) * NS, acc);
        operands();
        trip(std::true_type{}, (NTRIP - 1) * NS, Wnext, 0, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) *reinterpret_cast<f32x4*>(&part[kq][r][4 * c4]) = acc[r];
    };
    // Behind the last pass the ring's requests are dummies that nobody consumes; they may land until the wave ends, so
    // their registers must not be handed to anything else before: ring_end() keeps them the ring's up to that point.
    auto ring_end = [&]() {
        vm_wait<0>();
#pragma unroll
        for (int k = 0; k < RING; ++k) vm_landed(ring[k]);
    };
    // weight matrix of pass p: forward layers 2..L use Wh[0..L-2]; backward L..2 use WhT[L-2..0]
    const int n_pass = TRAIN ? 2 * (L - 1) : (L - 1);
    auto wseq = [&](int p) -> const float* {
        // The dummy behind the last pass is the first RING rows of every k-group of Wh[0]: rows kq * KPG + j < Hp of the
        // first hidden kernel, which exists at every width since L >= 2.  Every other request is a row of the matrix of
        // a pass that runs.  So every address of the stream lies inside Wh or WhT.
        if (p >= n_pass) return uniform_ptr(Wh);
        return uniform_ptr(p < L - 1 ? Wh + (int64_t)p * HH : WhT + (int64_t)(2 * (L - 1) - 1 - p) * HH);
    };
    auto ring_start = [&]() {
        const float* W0 = wseq(0);
#pragma unroll
        for (int s = 0; s < NS; ++s) load_slot(W0, s, s);
    };
    auto reduced = [&](int r, int n) {     // fixed-order sum over the k-groups
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < KG; ++g) s += part[g][r][n];
        return s;
    };

    // head operands: consumed after the forward chain.  The thread count is a multiple of the width, so element
    // i = t + SF_THREADS*o of the row block is column t % Hp for every o, and one pair of wa per thread serves the heads
    // (threads t < Hp) and the dz_L phase.
    static_assert(SF_THREADS % Hp == 0, "one pair of wa per thread needs a thread count that is a multiple of the width");
    float h_wa0 = 0.f, h_wa1 = 0.f;
    float h_ba0 = 0.f, h_ba1 = 0.f, h_w00 = 0.f, h_w01 = 0.f, h_w10 = 0.f, h_w11 = 0.f, h_bb0 = 0.f, h_bb1 = 0.f;
    float h_y0 = 0.f, h_y1 = 0.f;
    const bool has_y = Y != nullptr && t < R && r0 + t < n_b;

    // rows of this block: input of layer 2
    if (!TRAIN && rd_partial != nullptr) {
        // the many-row layer-1 GEMM left its SNP-group partial sums: the group sum + shift term + b1 + ELU that
        // l1_gemm_reduce_kernel would do in a launch of its own (33 MB read back by one kernel at 1000 and at 4096 rows)
        // happens here, spread over every row block of the stack launch.  Same association as that kernel - four
        // quarters of the groups, ((q0 + q1) + q2) + q3, then + (shift + b1) - so the activations are the same bits.
        // The group count is a run-time value, so these loads cannot all be requested ahead of the ring, and loads return
        // in order: a ring requested first would be drained by the first partial sum.  They stay the compiler's, in front
        // of every asm load; the ring starts behind them, in front of the barrier.
        const int gq = (rd_G + 3) / 4;
        for (int i = t; i < R * Hp; i += SF_THREADS) {
            const int r = i / Hp, n = i % Hp;
            float v = 0.f;
            if (r0 + r < n_b) {
                const float* src = rd_partial + (int64_t)(r0 + r) * Hp + n;
                float sq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int g0 = q * gq, g1 = g0 + gq < rd_G ? g0 + gq : rd_G;
                    float z = 0.f;
                    for (int g = g0; g < g1; ++g) z += src[(int64_t)g * rd_MH];
                    sq[q] = z;
                }
                float c = rd_cvec8[n];
#pragma unroll
                for (int sl = 1; sl < 8; ++sl) c += rd_cvec8[sl * Hp + n];
                v = elu_f((((sq[0] + sq[1]) + sq[2]) + sq[3]) + (c + rd_b1[n]));
            }
            act[r][n] = v;
        }
    }
    {
        // Everything the prologue needs is requested first and the ring right behind it: loads return in order, so the wait
        // in front of the staging covers exactly these and the first, coldest weight fetch runs beside the staging and the
        // barrier.
        const bool stage = TRAIN || rd_partial == nullptr;
        float a1v[NO];
        uint32_t yrow = 0;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int i = t + SF_THREADS * o;
            a1v[o] = 0.f;
            // inference: a1 is [n_b][Hp] and nothing beyond it is read - the rows of the last group past n_b (their results are
            // dropped) stage row n_b - 1 again.  The load itself stays unconditional: a predicate that is uniform over a row
            // could take a whole wave's load away.  The training launch carries every row of its 32-row blocks.
            int sr = r0 + i / Hp;
            if constexpr (!TRAIN) sr = sr < n_b ? sr : n_b - 1;
            if (stage && i < R * Hp) gload4_inout(a1v[o], a1_in + (int64_t)sr * Hp + i % Hp);
        }
        if (has_y) gload4_inout(yrow, rows + r0 + t);
        gload4_inout(h_wa0, wa + 2 * (t % Hp));
        gload4_inout(h_wa1, wa + 2 * (t % Hp) + 1);
        if (t < R) {
            gload4_inout(h_ba0, ba); gload4_inout(h_ba1, ba + 1);
            gload4_inout(h_w00, wb); gload4_inout(h_w01, wb + 1); gload4_inout(h_w10, wb + 2); gload4_inout(h_w11, wb + 3);
            gload4_inout(h_bb0, bb); gload4_inout(h_bb1, bb + 1);
        }
        ring_start();
        vm_wait<RING>();
#pragma unroll
        for (int o = 0; o < NO; ++o) vm_landed(a1v[o]);
        vm_landed(yrow);
        vm_landed(h_wa0); vm_landed(h_wa1);
        vm_landed(h_ba0); vm_landed(h_ba1); vm_landed(h_w00); vm_landed(h_w01); vm_landed(h_w10); vm_landed(h_w11);
        vm_landed(h_bb0); vm_landed(h_bb1);
        // the labels of this block's rows: younger than the ring's first requests, landed with the first pass's operands
        if (has_y) { gload4_inout(h_y0, Y + (int64_t)(int32_t)yrow * 2); gload4_inout(h_y1, Y + (int64_t)(int32_t)yrow * 2 + 1); }
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int i = t + SF_THREADS * o;
            if (stage && i < R * Hp) act[i / Hp][i % Hp] = a1v[o];
        }
    }
    lds_barrier();      // act is LDS: nothing here waits for the ring

    // ---------------- forward: layers 2..L
    for (int l = 2; l <= L; ++l) {
        const float* bias = bh + (int64_t)(l - 2) * Hp;
        const bool dr = TRAIN && mask != nullptr && l == n_pre;
        float e_bias[NO];
        uint32_t e_m[NO];
        contract(wseq(l - 2), wseq(l - 1), [&]() {
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                const int i = (t + SF_THREADS * o) % (R * Hp);
                e_bias[o] = 0.f;
                gload4_inout(e_bias[o], bias + i % Hp);
                e_m[o] = 1;
                if (dr) gload1_inout(e_m[o], mask + (int64_t)(r0 + i / Hp) * Hp + i % Hp);
            }
        });
        lds_barrier();
        vm_wait<RING>();        // the epilogue's operands: RING requests are younger
#pragma unroll
        for (int o = 0; o < NO; ++o) { vm_landed(e_bias[o]); vm_landed(e_m[o]); }
        vm_landed(h_y0); vm_landed(h_y1);
        float* aout = acts + (int64_t)(l - 1) * blk;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int i = t + SF_THREADS * o;
            if (i < R * Hp) {
                const int r = i / Hp, n = i % Hp;
                const float a = elu_f(reduced(r, n) + e_bias[o]);
                const int64_t gi = (int64_t)(r0 + r) * Hp + n;
                if (TRAIN) aout[gi] = a;
                float nx = a;
                if (dr) {
                    nx = a * (e_m[o] ? keep_scale : 0.f);
                    adrop[gi] = nx;
                }
                act[r][n] = nx;
            }
        }
        lds_barrier();
    }

    // ---------------- heads + loss (per row)
    {
        float p0[R], p1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { p0[r] = 0.f; p1[r] = 0.f; }
        if (t < Hp) {                   // Hp <= SF_THREADS: one k per thread
#pragma unroll
            for (int r = 0; r < R; ++r) { p0[r] = act[r][t] * h_wa0; p1[r] = act[r][t] * h_wa1; }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { p0[r] += __shfl_xor(p0[r], o); p1[r] += __shfl_xor(p1[r], o); }
            if ((t & 63) == 0) { part[0][r][2 * (t >> 6)] = p0[r]; part[0][r][2 * (t >> 6) + 1] = p1[r]; }
        }
        lds_barrier();
        if (t < R) {
            const int r = t, b = r0 + r;
            float y10 = h_ba0, y11 = h_ba1;
            for (int w = 0; w < SF_THREADS / 64; ++w) { y10 += part[0][r][2 * w]; y11 += part[0][r][2 * w + 1]; }
            const float w00 = h_w00, w01 = h_w01, w10 = h_w10, w11 = h_w11;
            const float y20 = y10 * w00 + y11 * w10 + h_bb0;
            const float y21 = y10 * w01 + y11 * w11 + h_bb1;
            float d = 0.f, g0 = 0.f, g1 = 0.f;
            const bool valid = b < n_b;
            if (valid && Y != nullptr) {
                const float e0 = y20 - h_y0, e1 = y21 - h_y1;
                d = sqrtf(fmaxf(TRAIN ? sf_sumsq_train(e0, e1) : sf_sumsq_eval(e0, e1), 0.f));
                if (d > 0.f) { g0 = e0 / d / (float)n_b; g1 = e1 / d / (float)n_b; }
            }
            if (TRAIN) {
                const float dy10 = g0 * w00 + g1 * w01, dy11 = g0 * w10 + g1 * w11;
                hs[r][0] = dy10; hs[r][1] = dy11;
                float* ho = head_out + 8 * b;       // [d, dy1_0, dy1_1, y1_0, y1_1, dy2_0, dy2_1, -]
                ho[0] = d; ho[1] = dy10; ho[2] = dy11; ho[3] = y10; ho[4] = y11; ho[5] = g0; ho[6] = g1; ho[7] = 0.f;
            } else if (valid) {
                yhat[2 * b] = y20; yhat[2 * b + 1] = y21;
                if (dist && Y != nullptr) dist[b] = d;      // no dist without targets (as loc_head_eval and stack_rows.hip)
            }
        }
        lds_barrier();
    }
    if (!TRAIN) {
        ring_end();
        return;
    }

    // ---------------- dz_L = (dy1 . Wa^T) * ELU'(a_L), then backward through layers L..2
    {
        float* dzo = dz + (int64_t)(L - 1) * blk;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int i = t + SF_THREADS * o;
            if (i < R * Hp) {
                const int r = i / Hp, k = i % Hp;           // wa[2k], wa[2k + 1]: in registers since the prologue
                const float v = (hs[r][0] * h_wa0 + hs[r][1] * h_wa1) * elu_grad_from_act(act[r][k]);
                dzo[(int64_t)(r0 + r) * Hp + k] = v;
                part[0][r][k] = v;     // staged; copied into act after the barrier (act is still being read)
            }
        }
        lds_barrier();
        for (int i = t; i < R * Hp; i += SF_THREADS) act[i / Hp][i % Hp] = part[0][i / Hp][i % Hp];
        lds_barrier();
    }
    for (int l = L; l >= 2; --l) {
        const int p = (L - 1) + (L - l);             // pass index of this backward layer
        const float* aprev = acts + (int64_t)(l - 2) * blk;      // ELU output of layer l-1 (pre-dropout)
        const bool dr = mask != nullptr && l - 1 == n_pre;
        float e_a[NO];
        uint32_t e_m[NO];
        // sum_n dz_l[r][n] * W_l[k][n] = dz_l . (W_l^T)[n][k]
        contract(wseq(p), wseq(p + 1), [&]() {
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                const int i = (t + SF_THREADS * o) % (R * Hp);
                const int64_t gi = (int64_t)(r0 + i / Hp) * Hp + i % Hp;
                e_a[o] = 0.f;
                gload4_inout(e_a[o], aprev + gi);
                e_m[o] = 1;
                if (dr) gload1_inout(e_m[o], mask + gi);
            }
        });
        lds_barrier();
        vm_wait<RING>();        // the epilogue's operands: RING requests are younger
#pragma unroll
        for (int o = 0; o < NO; ++o) { vm_landed(e_a[o]); vm_landed(e_m[o]); }
        float* dzo = dz + (int64_t)(l - 2) * blk;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int i = t + SF_THREADS * o;
            if (i < R * Hp) {
                const int r = i / Hp, k = i % Hp;
                float keep = 1.f;
                if (dr) keep = e_m[o] ? keep_scale : 0.f;
                const float v = reduced(r, k) * (keep * elu_grad_from_act(e_a[o]));
                dzo[(int64_t)(r0 + r) * Hp + k] = v;
                act[r][k] = v;
            }
        }
        lds_barrier();
    }
    ring_end();
}

// Everything that reduces over the batch rows, for all hidden layers at once: see stack_tail.h (stack_dw_all_body).
template <int NHT, int RB>
__global__ __launch_bounds__(512) void stack_dw_all_kernel(loc_dw_tail_args ta, loc_gb_tail gb) {
    stack_dw_all_body<NHT, RB>((int)blockIdx.x, ta, gb);
}

// hidden kernels -> transposed copies (after init / import / best-weight reload)
__global__ void transpose_hidden_kernel(const float* __restrict__ Wh, float* __restrict__ WhT, int Hp, int nl) {
    __shared__ float tile[32][33];
    const int l = blockIdx.z, bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* src = Wh + (int64_t)l * Hp * Hp;
    float* dst = WhT + (int64_t)l * Hp * Hp;
    for (int j = ty; j < 32; j += 8) tile[j][tx] = src[(int64_t)(by + j) * Hp + bx + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8) dst[(int64_t)(bx + j) * Hp + by + tx] = tile[tx][j];
    (void)nl;
}

extern "C" int loc_stack_fused_supported(int Hp) { return Hp == 64 || Hp == 128 || Hp == 256 || Hp == 512; }

#define SF_SWITCH(MACRO)                                                    \
    switch (Hp) {                                                           \
        case 64: MACRO(2); break;                                           \
        case 128: MACRO(4); break;                                          \
        case 256: MACRO(8); break;                                          \
        case 512: MACRO(16); break;                                         \
        default: loc_set_error("%s: fused stack needs width 64/128/256/512 after padding (got %d)", __func__, Hp); return -1; \
    }

extern "C" int loc_transpose_hidden(const float* Wh, float* WhT, int Hp, int n_hidden, void* stream) {
    if (n_hidden <= 0) return 0;
    hipLaunchKernelGGL(transpose_hidden_kernel, dim3(Hp / 32, Hp / 32, n_hidden), dim3(256), 0, (hipStream_t)stream, Wh,
                       WhT, Hp, n_hidden);
    LOC_CHECK_LAUNCH();
    return 0;
}

constexpr int SF_R = 2;   // batch rows per workgroup -> 16 workgroups per 32-row block
// rows per workgroup of the TRAINING launch (loc_tuning.stack_train_rows).  A worker is bound by its weight stream (4.7 MB of
// Wh + WhT from its XCD's L2) whatever its row count, and what a pass does between its last and the next pass's first slot -
// the reduction, two barriers, the epilogue - comes on top, longer with every row: measured at the metric's shape (bench.py,
// 32-row steps, 12 helpers, round 5) 4 rows per workgroup 189.9 us per step, 2 rows (rounds 1-4) 171.3, 1 row 162.4 (32 workers +
// helpers over two XCDs) - same bits.  One row per workgroup is ahead at every shape tried (profiles/r05_stack_train_rows.log):
// widths 64 / 128 / 512 +4 %, 5,830 SNPs +10 %, 20,000 +9 %, 500,000 +1 %, --batch_size 64 +1.7 %, 128 +0.8 %.  Round 7's register
// ring took the one-row kernel from 42.8 to 40.3 us (step 163.6 -> 161.2); the stream alone (no FMA, reduction, barrier or
// epilogue) is ~33 us, the L2 port's rate (profiles/r07_stack_stream_floor.txt).
static int sf_train_rows(const loc_tuning* tune, int n_b) {
    const int v = tune ? tune->stack_train_rows : 0;
    (void)n_b;
    return (v == 1 || v == 2 || v == 4) ? v : 1;
}

// L2 warm-up helper workgroups and XCD placement stride of the fused stack: speed hints (loc_tuning), defaults
// measured at width 256: helpers 0 -> 78.6 us, 4 -> 63, 8 -> 51.7, 12 -> 51.0, 32 -> 55 (round 3, two rows per workgroup);
// re-swept on the ring kernel (round 7, profiles/r07_stack_helpers.txt): 8 helpers 0.7 % behind 12, 16 and 20 within the
// repetitions' spread of 12, stride 4 = stride 8 - unchanged
static int sf_helpers(const loc_tuning* tune) {
    if (!tune || tune->stack_helpers == 0) return 12;
    return tune->stack_helpers < 0 ? 0 : tune->stack_helpers;
}
static int sf_xcd_stride(const loc_tuning* tune) {
    const int v = tune ? tune->stack_xcd_stride : 0;
    return v == 1 || v == 2 || v == 4 || v == 8 ? v : 8;
}

extern "C" int loc_stack_forward_backward(const float* a1_in, const float* Wh, const float* WhT, const float* bh,
                                          const float* wa, const float* ba, const float* wb, const float* bb,
                                          const uint8_t* mask, float keep_scale, int Hp, int L, int n_pre, int n_b,
                                          int slot_rows, const int32_t* rows, const float* Y, float* acts,
                                          float* adrop, float* dz, float* head_out, const loc_tuning* tune,
                                          void* stream) {
    // L >= 2: the kernel has at least one layer pass (the labels and the ring are waited for inside the passes)
    if (n_b < 1 || n_b > slot_rows || slot_rows % 32 || L < 2) {
        loc_set_error("loc_stack_forward_backward: n_b=%d, slot_rows=%d, L=%d", n_b, slot_rows, L);
        return -1;
    }
    // every row of the row blocks in use is carried (rows >= n_b get a zero loss gradient), so the tail and the
    // layer-1 backward can contract whole 32-row blocks
    const int rpw = sf_train_rows(tune, n_b);
    const int nblk = (n_b + 31) / 32 * (32 / rpw);
    int xs = sf_xcd_stride(tune);
    int nh = xs > 1 ? sf_helpers(tune) : 0;
    while (xs > 1 && (nblk + nh + 8 / xs - 1) / (8 / xs) > 32) {     // more row groups than one XCD holds
        xs /= 2;
        nh = (nh + 8 / xs - 1) / (8 / xs) * (8 / xs);
    }
    if (xs == 1) nh = 0;
#define LAUNCH_TR(N, RR)                                                                                           \
    hipLaunchKernelGGL((stack_fused_kernel<N, RR, true>), dim3((nblk + nh) * xs), dim3(SF_THREADS), 0,             \
                       (hipStream_t)stream, a1_in, Wh, WhT, bh, wa, ba, wb, bb, mask, keep_scale, L, n_pre, n_b,  \
                       rows, Y, acts, adrop, dz, head_out, (float*)nullptr, (float*)nullptr, xs, nblk, slot_rows,         \
                       (const float*)nullptr, 0, (int64_t)0, (const float*)nullptr, (const float*)nullptr);
#define LAUNCH1(N) LAUNCH_TR(N, 1)
#define LAUNCH2(N) LAUNCH_TR(N, 2)
#define LAUNCH4(N) LAUNCH_TR(N, 4)
    if (rpw == 1) { SF_SWITCH(LAUNCH1) } else if (rpw == 4) { SF_SWITCH(LAUNCH4) } else { SF_SWITCH(LAUNCH2) }
#undef LAUNCH1
#undef LAUNCH2
#undef LAUNCH4
#undef LAUNCH_TR
    LOC_CHECK_LAUNCH();
    return 0;
}

static int sf_eval_launch(const float* a1, const float* rd_partial, int rd_G, int64_t rd_MH, const float* rd_cvec8,
                          const float* rd_b1, const float* Wh, const float* bh, const float* wa, const float* ba,
                          const float* wb, const float* bb, int Hp, int L, int n_b, const int32_t* rows, const float* Y,
                          float* yhat, float* dist, void* stream, const char* who, int rows_form = 0) {
    // rows_form: 0 = by row count (width 256: 2, 4 or 8 rows per workgroup on the vector ALU while one round of workgroups
    // covers the rows, above 8 x compute units rows 16 or 32 rows per workgroup on the fp32 matrix pipe, stack_rows.hip: the
    // measured round times are there); 1 = always the 32-row matrix-pipe form (where supported), 2 = always the 16-row form;
    // -1 = always 2 rows per workgroup on the vector ALU, -2 = 4 rows, -3 = 8 rows (measurement / tests)
    // Refused on the host, before any launch (tests/test_gpu_stack_eval.py): L < 2 - the kernel has at least one layer pass (the
    // labels and the ring are waited for inside the passes); a width without a fused form; n_b < 0; targets without their row
    // indices or the reverse - every form would follow the one pointer it has on the device.
    if (L < 2 || !loc_stack_fused_supported(Hp) || n_b < 0 || (rows == nullptr) != (Y == nullptr) || !yhat ||
        (!a1 && !rd_partial) || !Wh || !bh || !wa || !ba || !wb || !bb) {
        loc_set_error("%s: Hp=%d (64/128/256/512 after padding) L=%d (>= 2) n_b=%d (>= 0) rows=%s Y=%s (both or neither)%s", who, Hp,
                      L, n_b, rows ? "given" : "NULL", Y ? "given" : "NULL",
                      yhat && (a1 || rd_partial) && Wh && bh && wa && ba && wb && bb ? "" : ", a NULL operand");
        return -1;
    }
    if (n_b == 0) return 0;      // nothing to do: no launch (the vector-ALU grid would hold warm-up helpers only)
    if (rows_form >= 0 && loc_stack_rows_supported(Hp, L) && (rows_form > 0 || n_b >= loc_stack_rows_min_rows()))
        return sr_eval_launch(a1, rd_partial, rd_G, rd_MH, rd_cvec8, rd_b1, Wh, bh, wa, ba, wb, bb, L, n_b, rows, Y, yhat, dist,
                              rows_form == 1 ? 32 : rows_form == 2 ? 16 : 0, stream);
    const loc_tuning* tune = nullptr;
    int rpw = SF_R;
    if (Hp == 256) {
        const int cu = sr_compute_units();
        if (rows_form == -2 || (rows_form == 0 && n_b > 2 * cu && n_b <= 4 * cu)) rpw = 4;
        else if (rows_form == -3 || (rows_form == 0 && n_b > 4 * cu)) rpw = 8;
    }
    const int nblk = (n_b + rpw - 1) / rpw;
    // Workers + warm-up helpers of one launch should be co-resident (32 CUs per XCD): with more row groups
    // than one XCD holds, spread them over 2, 4 or all 8 XCDs (stride 4, 2, 1) instead of running in rounds.
    int xs = sf_xcd_stride(tune);
    int nh = xs > 1 ? sf_helpers(tune) : 0;
    while (xs > 1 && (nblk + nh + 8 / xs - 1) / (8 / xs) > 32) {
        xs /= 2;
        nh = (nh + 8 / xs - 1) / (8 / xs) * (8 / xs);      // the same number of helpers on every XCD in use
    }
    if (xs == 1) nh = 0;
#define LAUNCH_R(N, RR)                                                                                           \
    hipLaunchKernelGGL((stack_fused_kernel<N, RR, false>), dim3((nblk + nh) * xs), dim3(SF_THREADS), 0,           \
                       (hipStream_t)stream, a1, Wh, (const float*)nullptr, bh, wa, ba, wb, bb,                    \
                       (const uint8_t*)nullptr, 1.f, L, 0, n_b, rows, Y, (float*)nullptr, (float*)nullptr,        \
                       (float*)nullptr, (float*)nullptr, yhat, dist, xs, nblk, 32, rd_partial, rd_G, rd_MH, rd_cvec8,  \
                       rd_b1);
#define LAUNCH(N) LAUNCH_R(N, SF_R)
    if (rpw == 4) { LAUNCH_R(8, 4) }
    else if (rpw == 8) { LAUNCH_R(8, 8) }

    else { SF_SWITCH(LAUNCH) }
#undef LAUNCH
#undef LAUNCH_R
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_stack_forward_eval(const float* a1, const float* Wh, const float* bh, const float* wa,
                                      const float* ba, const float* wb, const float* bb, int Hp, int L, int n_b,
                                      const int32_t* rows, const float* Y, float* yhat, float* dist, void* stream) {
    return sf_eval_launch(a1, nullptr, 0, 0, nullptr, nullptr, Wh, bh, wa, ba, wb, bb, Hp, L, n_b, rows, Y, yhat, dist, stream,
                          "loc_stack_forward_eval");
}
extern "C" int loc_stack_forward_eval_form(const float* a1, const float* Wh, const float* bh, const float* wa,
                                           const float* ba, const float* wb, const float* bb, int Hp, int L, int n_b,
                                           const int32_t* rows, const float* Y, float* yhat, float* dist, int rows_form,
                                           void* stream) {
    return sf_eval_launch(a1, nullptr, 0, 0, nullptr, nullptr, Wh, bh, wa, ba, wb, bb, Hp, L, n_b, rows, Y, yhat, dist, stream,
                          "loc_stack_forward_eval_form", rows_form);
}

extern "C" int loc_stack_forward_eval_partial(const float* partial, int groups, int64_t group_stride, const float* cvec8,
                                              const float* b1, const float* Wh, const float* bh, const float* wa,
                                              const float* ba, const float* wb, const float* bb, int Hp, int L, int n_b,
                                              const int32_t* rows, const float* Y, float* yhat, float* dist, int rows_form,
                                              void* stream) {
    if (!partial || groups < 1 || group_stride < (int64_t)n_b * Hp || !cvec8 || !b1) {
        loc_set_error("loc_stack_forward_eval_partial: groups=%d group_stride=%lld n_b=%d", groups, (long long)group_stride, n_b);
        return -1;
    }
    return sf_eval_launch(nullptr, partial, groups, group_stride, cvec8, b1, Wh, bh, wa, ba, wb, bb, Hp, L, n_b, rows, Y, yhat,
                          dist, stream, "loc_stack_forward_eval_partial", rows_form);
}

// the launcher on a filled argument block (step_args.h): an overload of the entry point, so that a refusal still names it
int loc_stack_dw_adam_tail(int Hp, const loc_dw_tail_args& ta, const loc_gb_tail* gb, void* stream) {
    const int L = ta.L, n_b = ta.n_b;
    if (n_b < 1 || n_b > LOC_BIG_BATCH_MAX || n_b > ta.slot_rows) {
        loc_set_error("loc_stack_dw_adam: n_b=%d (limit %d), slot_rows=%d", n_b, LOC_BIG_BATCH_MAX, ta.slot_rows);
        return -1;
    }
    const int nht = Hp / 32;
    loc_gb_tail g;
    if (gb) g = *gb; else { g = loc_gb_tail{}; g.K = 0; }
    const int grid = (L - 1) * nht * nht + 1 + (g.K > 0 ? (g.K + 511) / 512 : 0);
#define LAUNCH_RB(N, R) \
    hipLaunchKernelGGL((stack_dw_all_kernel<N, R>), dim3(grid), dim3(512), 0, (hipStream_t)stream, ta, g);
#define LAUNCH(N)                                                                                                 \
    switch ((n_b + 31) / 32) {                                                                                    \
        case 1: LAUNCH_RB(N, 1) break;                                                                            \
        case 2: LAUNCH_RB(N, 2) break;                                                                            \
        case 3: LAUNCH_RB(N, 3) break;                                                                            \
        case 4: LAUNCH_RB(N, 4) break;                                                                            \
        default: LAUNCH_RB(N, 0) break;   /* more than 128 rows: run-time block count */                          \
    }
    SF_SWITCH(LAUNCH)
#undef LAUNCH
#undef LAUNCH_RB
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_stack_dw_adam_tail(int Hp, int L, int n_pre, int n_b, int slot_rows, int use_drop, const float* acts,
                                      const float* adrop, const float* dz, const float* head_out, float* params,
                                      float* adam_m, float* adam_v, float* WhT, int64_t off_wh, int64_t off_bh,
                                      int64_t off_wa, int64_t off_ba, int64_t off_wb, int64_t off_bb,
                                      float* loss_out, const float* alpha_tab, int alpha_tab_len, const float* lr,
                                      const int* t_base, int t_off, const loc_gb_tail* gb, void* stream) {
    return loc_stack_dw_adam_tail(Hp, dw_tail_args_of(L, n_pre, n_b, slot_rows, use_drop, acts, adrop, dz, head_out, params,
                                                      adam_m, adam_v, WhT, off_wh, off_bh, off_wa, off_ba, off_wb, off_bb,
                                                      loss_out, {alpha_tab, alpha_tab_len, lr, t_base, t_off}),
                                  gb, stream);
}

extern "C" int loc_stack_dw_adam(int Hp, int L, int n_pre, int n_b, int use_drop, const float* acts,
                                 const float* adrop, const float* dz, const float* head_out, float* params,
                                 float* adam_m, float* adam_v, float* WhT, int64_t off_wh, int64_t off_bh,
                                 int64_t off_wa, int64_t off_ba, int64_t off_wb, int64_t off_bb, float* loss_out,
                                 const float* alpha_tab, int alpha_tab_len, const float* lr, const int* t_base,
                                 int t_off, void* stream) {
    return loc_stack_dw_adam_tail(Hp, L, n_pre, n_b, 32, use_drop, acts, adrop, dz, head_out, params, adam_m, adam_v, WhT,
                                  off_wh, off_bh, off_wa, off_ba, off_wb, off_bb, loss_out, alpha_tab, alpha_tab_len,
                                  lr, t_base, t_off, nullptr, stream);
}
