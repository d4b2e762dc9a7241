// Identity-by-descent segments of the ibd command (locator_amd/ibd.py): loc_ibd_pack, loc_ibd_scan and loc_ibd_fill, defined in
// include/locator_hip_ibd.h; the NumPy forms ibd.pack_host and ibd.segments_host are what tests/test_gpu_ibd.py holds them to,
// bit for bit.  Integer code throughout: no float, no atomics, no LDS.
//
// ibd_pack_kernel: a thread packs 64 sites of four consecutive columns, one dword of a site's row a load (a wave reads 256
// consecutive bytes of a row), and stores the allele and the valid word of each column.
// ibd_scan_kernel<FILL>: one lane a pair (p, q).  A workgroup holds LOC_IBD_BLOCK consecutive q (the word-major planes [w][q]
// load coalesced, 8 bytes a lane and plane) against one row p, whose two words and the chromosome-start word of a step are
// wave-uniform and come through the scalar cache.  blockIdx.x is the row, so that the workgroups in flight together walk the
// same 256 columns and share their words in L2.  A step forms disc = (a_p ^ a_q) & v_p & v_q and visits the set bits of
// disc | first only; a word without one costs the loads and four operations.  The pair's state is a handful of registers:
// where the current run began, the open chain (its start, the end of its last run, the two coordinates, the seed flag) and the
// totals.  ibd_walk is the one device function behind both entry points: the count pass and the fill pass differ in what
// `emit` does with a finished segment and in nothing else.
#include "common.h"
#include "pair_tiles.h"

#include "../../include/locator_hip_ibd.h"

#include <cstdint>

constexpr int IB_BLOCK = LOC_IBD_BLOCK;
constexpr int IB_COLS = LOC_IBD_PACK_COLS;
static_assert(IB_BLOCK % 64 == 0 && IB_COLS == 4, "whole waves; a dword of alleles a thread");

struct ib_params { int64_t seed_sites, seed_len, extend_sites, gap_sites, gap_len, min_len; };

// ---------------------------------------------------------------------------------------------------------------- pack
__global__ __launch_bounds__(256) void ibd_pack_kernel(const int8_t* __restrict__ h, int H, int64_t K, int64_t pitch,
                                                       uint64_t* __restrict__ bits, int64_t wpitch, int64_t W) {
    const int64_t d0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * IB_COLS;
    const int64_t w = blockIdx.y;
    if (d0 >= wpitch) return;
    uint64_t al[IB_COLS] = {0, 0, 0, 0}, va[IB_COLS] = {0, 0, 0, 0};
    if (d0 < H) {                                                    // pitch >= H and a multiple of 16: the dword is inside the row
        const int64_t j0 = w * 64;
        const int n = (int)(K - j0 < 64 ? K - j0 : 64);
        const int8_t* src = h + j0 * pitch + d0;
        for (int t = 0; t < n; ++t) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (int64_t)t * pitch);
#pragma unroll
            for (int c = 0; c < IB_COLS; ++c) {
                const int a = (int)(v << (24 - 8 * c)) >> 24;
                al[c] |= (uint64_t)(a > 0) << t;
                va[c] |= (uint64_t)(a >= 0) << t;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < IB_COLS; ++c) {
        const int64_t d = d0 + c;
        if (d < wpitch) {
            const bool real = d < H;                                 // a pad column of h is never interpreted
            bits[w * wpitch + d] = real ? al[c] : 0;
            bits[(W + w) * wpitch + d] = real ? va[c] : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- scan
struct ib_state {
    int64_t ch_xa, ch_xb;      // x of the open chain's first site and of its last run's end
    int64_t length, longest;
    int rs;                    // the site after the last separator: where the current run begins
    int ch_a, ch_b;            // the open chain: its first site, the end of its last run
    int count;
    bool open, seed;
};

template <bool FILL>
__device__ __forceinline__ void ib_finish(ib_state& s, const ib_params& P, int64_t base, int64_t capacity, int32_t* seg_a,
                                          int32_t* seg_b) {
    if (s.open && s.seed) {
        const int64_t len = s.ch_xb - s.ch_xa;
        if (len >= P.min_len) {
            if (FILL) {
                const int64_t at = base + s.count;
                if (at >= 0 && at < capacity) {
                    seg_a[at] = s.ch_a;
                    seg_b[at] = s.ch_b;
                }
            }
            s.count += 1;
            s.length += len;
            s.longest = len > s.longest ? len : s.longest;
        }
    }
    s.open = false;
}

// the run [a, b] has ended (b >= a): it joins the open chain, or ends it and opens the next
template <bool FILL>
__device__ __forceinline__ void ib_close_run(ib_state& s, int a, int b, const int64_t* __restrict__ x, const ib_params& P,
                                             int64_t base, int64_t capacity, int32_t* seg_a, int32_t* seg_b) {
    const int64_t n = (int64_t)b - a + 1;
    if (n < P.extend_sites) {                    // links to nothing and, as extend_sites <= seed_sites, is no seed: a chain alone
        ib_finish<FILL>(s, P, base, capacity, seg_a, seg_b);
        return;
    }
    const int64_t xa = x[a], xb = x[b];
    const bool seed = n >= P.seed_sites && xb - xa >= P.seed_len;
    const int64_t g = (int64_t)a - s.ch_b - 1;
    // a first site in ch_b + 1 .. a has closed the chain on the way (ib_walk), so `open` stands for the rule's third condition
    if (s.open && g >= 1 && g <= P.gap_sites && xa - s.ch_xb <= P.gap_len) {
        s.ch_b = b;
        s.ch_xb = xb;
        s.seed = s.seed || seed;
        return;
    }
    ib_finish<FILL>(s, P, base, capacity, seg_a, seg_b);
    s.open = true;
    s.seed = seed;
    s.ch_a = a;
    s.ch_b = b;
    s.ch_xa = xa;
    s.ch_xb = xb;
}

// the whole walk of one pair over the W words; q's words at aq[w * wpitch], vq[w * wpitch], p's (wave-uniform) at ap, vp
template <bool FILL>
__device__ __forceinline__ void ib_walk(ib_state& s, const uint64_t* __restrict__ ap, const uint64_t* __restrict__ vp,
                                        const uint64_t* __restrict__ aq, const uint64_t* __restrict__ vq, int64_t wpitch, int64_t W,
                                        int64_t K, const uint64_t* __restrict__ first_bits, const int64_t* __restrict__ x,
                                        const ib_params& P, int64_t base, int64_t capacity, int32_t* seg_a, int32_t* seg_b) {
    s.open = false;
    s.seed = false;
    s.rs = 0;
    s.ch_a = s.ch_b = 0;
    s.count = 0;
    s.ch_xa = s.ch_xb = s.length = s.longest = 0;
    const uint64_t tail = (K & 63) ? (((uint64_t)1 << (K & 63)) - 1) : ~(uint64_t)0;
    uint64_t na = aq[0], nv = vq[0];
    for (int64_t w = 0; w < W; ++w) {
        const uint64_t qa = na, qv = nv;
        if (w + 1 < W) {                          // the next step's words are asked for before this step's bits are walked
            na = aq[(w + 1) * wpitch];
            nv = vq[(w + 1) * wpitch];
        }
        const uint64_t pa = ap[w * wpitch], pv = vp[w * wpitch], fb = first_bits[w];
        const uint64_t disc = (pa ^ qa) & pv & qv;
        uint64_t ev = disc | fb;
        if (w == W - 1) ev &= tail;               // no event at a site >= K, whatever the words hold there: x ends at K - 1
        while (ev) {
            const int t = __builtin_ctzll(ev);
            ev &= ev - 1;
            const int e = (int)(w * 64) + t;
            if (e > s.rs) ib_close_run<FILL>(s, s.rs, e - 1, x, P, base, capacity, seg_a, seg_b);
            if ((fb >> t) & 1) ib_finish<FILL>(s, P, base, capacity, seg_a, seg_b);        // nothing links across a chromosome start
            s.rs = e + (int)((disc >> t) & 1);
        }
    }
    if ((int64_t)s.rs < K) ib_close_run<FILL>(s, s.rs, (int)(K - 1), x, P, base, capacity, seg_a, seg_b);
    ib_finish<FILL>(s, P, base, capacity, seg_a, seg_b);
}

template <bool FILL>
__global__ __launch_bounds__(IB_BLOCK) void ibd_scan_kernel(const uint64_t* __restrict__ bits, int64_t wpitch, int H, int64_t K,
                                                            int64_t W, const int32_t* __restrict__ owner,
                                                            const uint64_t* __restrict__ first_bits, const int64_t* __restrict__ x,
                                                            int p0, ib_params P, int32_t* __restrict__ count,
                                                            int64_t* __restrict__ length, int64_t* __restrict__ longest,
                                                            const int64_t* __restrict__ offsets, int64_t capacity,
                                                            int32_t* __restrict__ seg_a, int32_t* __restrict__ seg_b) {
    const int i = blockIdx.x;
    const int p = p0 + i;
    const int q = (int)blockIdx.y * IB_BLOCK + (int)threadIdx.x;
    if (q >= H) return;
    const int64_t at = (int64_t)i * H + q;
    ib_state s;
    s.count = 0;
    s.length = s.longest = 0;
    if (q > p && owner[q] != owner[p]) {
        const uint64_t* alleles = bits;
        const uint64_t* valid = bits + W * wpitch;
        ib_walk<FILL>(s, alleles + p, valid + p, alleles + q, valid + q, wpitch, W, K, first_bits, x, P, FILL ? offsets[at] : 0,
                      capacity, seg_a, seg_b);
    }
    if (!FILL) {
        count[at] = s.count;
        length[at] = s.length;
        longest[at] = s.longest;
    }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
static bool ib_sizes_ok(const char* who, int H, int64_t K, int64_t wpitch) {
    if (H < 1 || H > LOC_IBD_MAX_HAPS || K < 0 || K >= ((int64_t)1 << 31) || wpitch < H || wpitch % 8 != 0) {
        loc_set_error("%s: H=%d K=%lld wpitch=%lld (H 1 .. %d; K 0 .. 2^31 - 1; wpitch >= H and a multiple of 8)", who, H, (long long)K,
                      (long long)wpitch, LOC_IBD_MAX_HAPS);
        return false;
    }
    return true;
}

extern "C" int loc_ibd_pack(const int8_t* h, int H, int64_t K, int64_t pitch, uint64_t* bits, int64_t wpitch, void* stream) {
    if (!ib_sizes_ok("loc_ibd_pack", H, K, wpitch)) return -1;
    if (pitch < H) {
        loc_set_error("loc_ibd_pack: pitch=%lld below H=%d", (long long)pitch, H);
        return -1;
    }
    if (!pt_rows_aligned("loc_ibd_pack", h, pitch)) return -1;
    if (K == 0) return 0;
    if (!h || !bits || (uintptr_t)bits % 8 != 0) {
        loc_set_error("loc_ibd_pack: h and bits must not be null, bits a multiple of 8 bytes");
        return -1;
    }
    const int64_t W = (K + 63) / 64;
    const int64_t groups = (wpitch + IB_COLS - 1) / IB_COLS;
    // grid.y holds at most 65535 blocks: the words go in slices, each a launch over (column groups, words of the slice)
    for (int64_t w0 = 0; w0 < W; w0 += LOC_GRID_Y_MAX) {
        const int64_t nw = W - w0 < LOC_GRID_Y_MAX ? W - w0 : LOC_GRID_Y_MAX;
        const int64_t Ks = K - w0 * 64;
        hipLaunchKernelGGL(ibd_pack_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)nw), dim3(256), 0, (hipStream_t)stream,
                           h + w0 * 64 * pitch, H, Ks, pitch, bits + w0 * wpitch, wpitch, W);
        LOC_CHECK_LAUNCH();
    }
    return 0;
}

static bool ib_scan_args_ok(const char* who, const uint64_t* bits, int64_t wpitch, int H, int64_t K, const int32_t* owner,
                            const uint64_t* first_bits, const int64_t* x, int p0, int R, const ib_params& P) {
    if (!ib_sizes_ok(who, H, K, wpitch)) return false;
    if (p0 < 0 || R < 0 || (int64_t)p0 + R > H) {
        loc_set_error("%s: p0=%d R=%d (rows p0 .. p0 + R - 1 must be columns 0 .. %d)", who, p0, R, H - 1);
        return false;
    }
    if (P.seed_sites < 1 || P.extend_sites < 1 || P.extend_sites > P.seed_sites || P.gap_sites < 0 || P.gap_sites > LOC_IBD_MAX_GAP ||
        P.seed_len < 0 || P.gap_len < 0 || P.min_len < 0) {
        loc_set_error("%s: seed_sites=%lld seed_len=%lld extend_sites=%lld gap_sites=%lld gap_len=%lld min_len=%lld (seed_sites >= 1, "
                      "1 <= extend_sites <= seed_sites, 0 <= gap_sites <= %d, no length negative)", who, (long long)P.seed_sites,
                      (long long)P.seed_len, (long long)P.extend_sites, (long long)P.gap_sites, (long long)P.gap_len,
                      (long long)P.min_len, LOC_IBD_MAX_GAP);
        return false;
    }
    if (R > 0 && K > 0 && (!bits || !owner || !first_bits || !x)) {
        loc_set_error("%s: null buffer", who);
        return false;
    }
    if ((uintptr_t)bits % 8 != 0 || (uintptr_t)first_bits % 8 != 0 || (uintptr_t)x % 8 != 0 || (uintptr_t)owner % 4 != 0) {
        loc_set_error("%s: bits, first_bits and x must be multiples of 8 bytes, owner of 4", who);
        return false;
    }
    return true;
}

extern "C" int loc_ibd_scan(const uint64_t* bits, int64_t wpitch, int H, int64_t K, const int32_t* owner, const uint64_t* first_bits,
                            const int64_t* x, int p0, int R, int64_t seed_sites, int64_t seed_len, int64_t extend_sites,
                            int64_t gap_sites, int64_t gap_len, int64_t min_len, int32_t* count, int64_t* length, int64_t* longest,
                            void* stream) {
    const ib_params P = {seed_sites, seed_len, extend_sites, gap_sites, gap_len, min_len};
    if (!ib_scan_args_ok("loc_ibd_scan", bits, wpitch, H, K, owner, first_bits, x, p0, R, P)) return -1;
    if (R == 0) return 0;
    if (!count || !length || !longest || (uintptr_t)count % 4 != 0 || (uintptr_t)length % 8 != 0 || (uintptr_t)longest % 8 != 0) {
        loc_set_error("loc_ibd_scan: count, length and longest must not be null, count a multiple of 4 bytes, the others of 8");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (K == 0) {
        const size_t n = (size_t)R * (size_t)H;
        hipError_t e = hipMemsetAsync(count, 0, n * sizeof(int32_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(length, 0, n * sizeof(int64_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(longest, 0, n * sizeof(int64_t), s);
        if (e != hipSuccess) {
            loc_set_error("loc_ibd_scan: %s", hipGetErrorString(e));
            return -1;
        }
        return 0;
    }
    hipLaunchKernelGGL(ibd_scan_kernel<false>, dim3((unsigned)R, (unsigned)((H + IB_BLOCK - 1) / IB_BLOCK)), dim3(IB_BLOCK), 0, s, bits,
                       wpitch, H, K, (K + 63) / 64, owner, first_bits, x, p0, P, count, length, longest, (const int64_t*)nullptr,
                       (int64_t)0, (int32_t*)nullptr, (int32_t*)nullptr);
    LOC_CHECK_LAUNCH();
    return 0;
}

extern "C" int loc_ibd_fill(const uint64_t* bits, int64_t wpitch, int H, int64_t K, const int32_t* owner, const uint64_t* first_bits,
                            const int64_t* x, int p0, int R, int64_t seed_sites, int64_t seed_len, int64_t extend_sites,
                            int64_t gap_sites, int64_t gap_len, int64_t min_len, const int64_t* offsets, int64_t capacity,
                            int32_t* seg_a, int32_t* seg_b, void* stream) {
    const ib_params P = {seed_sites, seed_len, extend_sites, gap_sites, gap_len, min_len};
    if (!ib_scan_args_ok("loc_ibd_fill", bits, wpitch, H, K, owner, first_bits, x, p0, R, P)) return -1;
    if (capacity < 0) {
        loc_set_error("loc_ibd_fill: capacity=%lld is negative", (long long)capacity);
        return -1;
    }
    if (R == 0 || K == 0 || capacity == 0) return 0;
    if (!offsets || !seg_a || !seg_b || (uintptr_t)offsets % 8 != 0 || (uintptr_t)seg_a % 4 != 0 || (uintptr_t)seg_b % 4 != 0) {
        loc_set_error("loc_ibd_fill: offsets, seg_a and seg_b must not be null, offsets a multiple of 8 bytes, the others of 4");
        return -1;
    }
    hipLaunchKernelGGL(ibd_scan_kernel<true>, dim3((unsigned)R, (unsigned)((H + IB_BLOCK - 1) / IB_BLOCK)), dim3(IB_BLOCK), 0,
                       (hipStream_t)stream, bits, wpitch, H, K, (K + 63) / 64, owner, first_bits, x, p0, P, (int32_t*)nullptr,
                       (int64_t*)nullptr, (int64_t*)nullptr, offsets, capacity, seg_a, seg_b);
    LOC_CHECK_LAUNCH();
    return 0;
}
