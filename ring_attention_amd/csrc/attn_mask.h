// Attention mask geometry: the ONE place that knows the algebra.
//
//   attend(i, j) <=> (!causal || j <= qpos(i)) && (!has_win || qpos(i) - j <= win)
//   qpos(i) = i * q_stride + diag
//
// (the host folds ring-rank offsets and layout strides into diag / q_stride /
// win — docs/KERNELS.md section 1).  The forward, dq, dkv and fp8 forward
// kernels, the launchers, the bindings and (through the bindings) the Python
// descriptor builder all take their tile shapes, tile ranges, grid.z shares,
// full-tile test and per-element test from here.  Plain C++17: device code
// sees __host__ __device__ __forceinline__, bindings.cpp plain inline.
#pragma once

#ifdef __HIPCC__
#define RING_ATTN_MASK_FN __host__ __device__ __forceinline__
#else
#define RING_ATTN_MASK_FN inline
#endif

namespace ring_attn {

// ---- tile shapes
constexpr int ROWS_WG = 256;      // owner rows per workgroup: q rows (fwd, dq,
                                  // fp8) or kv rows (dkv); 8 waves x 32 rows
constexpr int kvblk(int d) { return d == 64 ? 128 : 64; }   // fwd / dq kv tile
                                                             // (LDS budget)
constexpr int DKV_QT = 64;        // dkv q tile, every head dim
// KVBLK 256 measured NEGATIVE and wrong (profiles/README.md) — keep 128
constexpr int FP8_KVBLK = 128;    // fp8 forward kv tile, every head dim

constexpr long ceil_div(long a, long b) { return (a + b - 1) / b; }

struct TileRange { int lo, hi; };   // tiles [lo, hi)
struct RowCut { int lo, hi; };      // key offsets [lo, hi] of one tile, inclusive

struct Mask {
    int causal, has_win;
    long diag, q_stride, win;

    RING_ATTN_MASK_FN long qpos(long i) const { return i * q_stride + diag; }

    // per-element test for a q position and a key; `ok` carries the caller's
    // own terms (ragged tail, row validity) in and the conjunction out.  Keep
    // this form: `ok && attends(qp, j)` with the conjunction built here
    // compiles to 28-72 B/lane more scratch in the plain dkv instantiations.
    RING_ATTN_MASK_FN bool attends(long qp, long j, bool ok = true) const {
        if (causal) ok = ok && (j <= qp);
        if (has_win) ok = ok && (qp - j <= win);
        return ok;
    }

    // the per-element test of one q position against the W keys of the tile
    // that starts at j0, reduced to 32-bit offsets: key j0 + o (0 <= o < W)
    // attends  <=>  lo <= o <= hi  <=>  attends(qp, j0 + o, j0 + o < nk).
    // All 64-bit arithmetic happens here, once per (row, tile); an empty
    // row gives lo > hi.
    RING_ATTN_MASK_FN RowCut row_cut(long qp, long j0, int W, long nk) const {
        long hi = nk - 1 - j0, lo = 0;
        if (hi > W - 1) hi = W - 1;
        if (causal && qp - j0 < hi) hi = qp - j0;
        if (has_win && qp - win - j0 > lo) lo = qp - win - j0;
        if (hi < -1) hi = -1;
        if (lo > W) lo = W;
        return {(int)lo, (int)hi};
    }

    // no pair of (q positions [q_lo, q_hi]) x (keys [j0, jmax]) is cut by
    // causal or window.  The test is symmetric, so it serves both walks: a
    // kv tile against the workgroup's q rows, a q tile against its keys.
    RING_ATTN_MASK_FN bool uncut(long q_lo, long q_hi, long j0, long jmax) const {
        return (!causal || jmax <= q_lo) && (!has_win || (q_hi - j0) <= win);
    }

    // kv tiles of width W that q rows [i_min, i_max] can attend: the masked
    // region is contiguous, so the range is computed once per workgroup
    RING_ATTN_MASK_FN TileRange kv_tile_range(long i_min, long i_max, long nk, int W) const {
        const long q_min = qpos(i_min), q_max = qpos(i_max);
        const int n = (int)((nk + W - 1) / W);
        TileRange r{0, n};
        if (causal) {
            const long t = q_max / W + 1;
            r.hi = q_max < 0 ? 0 : (int)(t < (long)n ? t : (long)n);
        }
        if (has_win) {
            // tile t attends iff j0 + W - 1 >= q_min - win
            const long x = q_min - win - W + 1;
            r.lo = x <= 0 ? 0 : (int)((x + W - 1) / W);
            if (r.lo > r.hi) r.lo = r.hi;
        }
        return r;
    }

    // q tiles of width W that hold a row attending one of keys [j0, jmax]
    RING_ATTN_MASK_FN TileRange q_tile_range(long j0, long jmax, long nq, int W) const {
        const int n = (int)((nq + W - 1) / W);
        TileRange r{0, n};
        if (causal) {
            // need qpos(i) >= j0  =>  i >= (j0 - diag) / q_stride
            const long i_min_needed = (j0 - diag + q_stride - 1) / q_stride;
            if (i_min_needed > 0) r.lo = (int)(i_min_needed / W);
        }
        if (has_win) {
            // need qpos(i) <= jmax + win  =>  i <= (jmax + win - diag) / q_stride
            const long num = jmax + win - diag;
            const long i_max_needed = num < 0 ? -1 : num / q_stride;
            if (i_max_needed < (long)n * W) {
                const long t = i_max_needed < 0 ? 0 : i_max_needed / W + 1;
                r.hi = (int)(t < (long)n ? t : (long)n);
            }
        }
        if (r.lo > r.hi) r.lo = r.hi;   // keys no row reaches: empty walk
        return r;
    }
};

// grid.z share z of `splits`: a fractional split of the workgroup's OWN valid
// range (a global-range split is skewed against the causal trapezoid)
RING_ATTN_MASK_FN TileRange split_share(TileRange r, int splits, int z) {
    const int valid = r.hi - r.lo;
    const int per = (valid + splits - 1) / splits;
    const int a = z * per, b = (z + 1) * per;
    return {r.lo + (valid < a ? valid : a), r.lo + (valid < b ? valid : b)};
}

// every params struct spells the geometry with the same five fields
template <class P>
RING_ATTN_MASK_FN Mask mask_of(const P& p) {
    return {p.causal, p.has_win, p.diag, p.q_stride, p.win};
}

}  // namespace ring_attn
