// gb_mxv.hip -- masked SpMV over a semiring: the kernels behind GrB_mxv and
// GrB_vxm (replaces SuiteSparse's GB_AxB dot/saxpy kernels reached from
// reference core/matrix.py:2196 and core/vector.py:1298).
//
// Pull (bottom-up): output position r reads row r of A' (CSR for mxv, the
// cached CSC for vxm), tests the bitmap of u for each column k and folds the
// products with the monoid.  Masked-out rows are skipped before any of their
// entries are read (the BFS `~v.S` mask removes every visited vertex).
// Monoids with a terminal value (LOR, ANY, MIN on integers, ...) stop a row as
// soon as any lane of its group reaches it.
// Layout: a 256-thread block owns tiles of 256 consecutive output rows
// (4 bitmap words).  G lanes (G = 1..64) share a row; their column-index loads
// are coalesced.  Output presence bits are assembled in LDS and written as
// whole 64-bit words; one counter atomic per block.
//
// That is k_spmv_pull, the fallback for operands that are not matrix objects.
// Matrices take k_spmv_words (balanced output words, see below) with
// k_spmv_fold for their long rows and k_hot_gather for a dense u's hot columns.
// These kernels are templates over the semiring (gb_dispatch_sr).
//
// Iso results (BFS lor_land / any_pair: only presence is computed, see
// gb_spmv_result_iso) do not come through here: gb_spmv hands them to
// gb_spmv_iso (gb_spmv_iso.hip), the direction-optimised push/pull path -- by
// default one k_iso_work launch per call, preceded by k_dir_prep only when the
// direction has to be decided from a frontier edge count nobody has yet.
//
// The per-orientation caches the kernels of both files read (hub chunks, pull
// heads, non-empty rows, long-row chunks) are built here: gb_view_*.
#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define SPMV_TILE 256

template <class SR, class X, class Z, bool FLIP>
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_pull(
    SR sr, int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    const X *__restrict__ avals, bool a_iso, const uint64_t *__restrict__ ubits,
    const X *__restrict__ uvals, bool u_iso, const uint64_t *__restrict__ mbits, bool mcomp, int lg,
    uint64_t *__restrict__ tbits, Z *__restrict__ tvals, unsigned long long *__restrict__ tcount,
    unsigned long long *__restrict__ gst) {
    __shared__ unsigned long long words[SPMV_TILE / 64];
    const int G = 1 << lg;
    const int gid = threadIdx.x >> lg;
    const int gl = threadIdx.x & (G - 1);
    const int ngroups = SPMV_BLOCK >> lg;
    const int lane = threadIdx.x & 63;
    const unsigned long long gmask = (G == 64) ? ~0ULL : (((1ULL << G) - 1) << (lane & ~(G - 1)));
    const int64_t nwords = (nrows + 63) >> 6;
    const bool rv = SR::reads_values && avals && uvals;
    X a0 = X(), u0 = X();
    if (rv) {
        if (a_iso) a0 = avals[0];
        if (u_iso) u0 = uvals[0];
    }
    unsigned long long mycount = 0;
    for (int64_t tile = blockIdx.x; tile * SPMV_TILE < nrows; tile += gridDim.x) {
        if (threadIdx.x < SPMV_TILE / 64) words[threadIdx.x] = 0;
        __syncthreads();
        const int64_t base = tile * SPMV_TILE;
        for (int rr = gid; rr < SPMV_TILE; rr += ngroups) {
            const int64_t r = base + rr;
            bool active = r < nrows;
            if (active && mbits) active = gb_bit(mbits, r) != mcomp;
            bool found = false;
            Z acc = Z();
            if (active) {
                const int64_t p1 = rowptr[r + 1];
                for (int64_t p = rowptr[r] + gl; p < p1; p += G) {
                    const int k = colidx[p];
                    bool term = false;
                    if (gb_bit(ubits, k)) {
                        X a = X(), b = X();
                        if (rv) {
                            a = a_iso ? a0 : avals[p];
                            b = u_iso ? u0 : uvals[k];
                        }
                        Z z = FLIP ? sr.mult(b, a, 0, k, r) : sr.mult(a, b, r, k, 0);
                        acc = found ? sr.add(acc, z) : z;
                        found = true;
                        term = sr.terminal(acc);
                    }
                    if (__ballot(term) & gmask) break;
                }
            }
            // reduce the group's partial results (all lanes reconverged here)
            for (int off = G >> 1; off > 0; off >>= 1) {
                bool of = __shfl_xor((int)found, off, 64);
                Z oa = gb_shfl_xor(acc, off, 64);
                if (of) {
                    acc = found ? ((gl & off) ? sr.add(oa, acc) : sr.add(acc, oa)) : oa;
                    found = true;
                }
            }
            if (gl == 0 && found) {
                if (tvals) tvals[r] = acc;
                atomicOr(&words[rr >> 6], 1ULL << (rr & 63));
            }
        }
        __syncthreads();
        if (threadIdx.x < SPMV_TILE / 64) {
            const int64_t w = (base >> 6) + threadIdx.x;
            if (w < nwords) {
                unsigned long long bitsw = words[threadIdx.x];
                tbits[w] = bitsw;
                mycount += __popcll(bitsw);
            }
        }
    }
    gb_grid_add(threadIdx.x < SPMV_TILE / 64 ? (long long)mycount : 0, tcount, gst);
}

// ------------------------------------------------ general SpMV: balanced words
// One wave per 64-row output word (a bitmap word): the entries of the word's
// rows (rows of at most LONG entries) are concatenated and walked 256 at a
// time, four independent gathers per lane; products of one row sit in
// consecutive lanes, so a segmented scan across the wave folds them and the
// last lane of each segment adds the run to the row's accumulator in LDS (row
// order = ascending k: deterministic).  Rows longer than LONG are cut into
// CH-entry chunks (a table cached on the matrix) whose partial folds are
// combined in chunk order by k_spmv_fold.
#define SPMV_LONG 128
#define SPMV_CH 1024
#define SPMV_WU 8  // entries per lane per step of the words kernel (gathers in flight)

template <class SR, class X, class Z, bool FLIP>
__device__ __forceinline__ void gb_spmv_product(SR &sr, bool rv, const X *__restrict__ avals, bool a_iso, X a0,
                                                const X *__restrict__ uvals, bool u_iso, X u0, int64_t p, int k,
                                                int64_t r, Z &z, const X *__restrict__ uhot, bool nt = false) {
    X a = X(), b = X();
    if (rv) {
        // nt: the streamed A values bypass L2 retention (the hot x values stay resident)
        a = a_iso ? a0 : (nt ? __builtin_nontemporal_load(&avals[p]) : avals[p]);
        // k < 0: a hot column (relabelled colidx, gb_view_hot): its value from the packed copy
        b = u_iso ? u0 : (k < 0 ? uhot[k & 0x7fffffff] : uvals[k]);
    }
    z = FLIP ? sr.mult(b, a, 0, k, r) : sr.mult(a, b, r, k, 0);
}

// Merge-path word (general SpMV, mode 1): the word's concatenated entries are
// cut into 64 equal contiguous runs, one per lane; a lane folds its run
// sequentially (row changes read from LDS, four entries' loads issued ahead),
// rows wholly inside one run are finished by that lane, and rows crossing runs
// are folded by their owner lane from the runs' carries in lane order.
template <class Z>
struct gb_mp_lds {
    int incl[64];
    int64_t p0[64];
    Z pa[64], pb[64];  // carry of the row continuing from the previous run / into the next
    int fa[64], fb[64];
};

template <class SR, class X, class Z, bool FLIP>
__device__ __forceinline__ long long gb_spmv_words_mp(
    SR &sr, int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    const X *__restrict__ avals, bool a_iso, X a0, const uint64_t *__restrict__ ubits, const X *__restrict__ uvals,
    bool u_iso, X u0, const uint64_t *__restrict__ mbits, bool mcomp, bool ufull, bool rv,
    uint64_t *__restrict__ tbits, Z *__restrict__ tvals, Z *acc, int *fl, gb_mp_lds<Z> &M,
    const X *__restrict__ uhot) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nwords = (nrows + 63) >> 6;
    long long cnt = 0;
    for (int64_t w = wave; w < nwords; w += nwaves) {
        const int64_t r = (w << 6) + lane;
        bool open = r < nrows;
        if (open && mbits) open = gb_bit(mbits, r) != mcomp;
        int64_t p0 = 0;
        int len = 0;
        if (open) {
            p0 = rowptr[r];
            const int64_t d = rowptr[r + 1] - p0;
            len = d > SPMV_LONG ? 0 : (int)d;  // long rows: chunks + k_spmv_fold
        }
        int incl = len;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        const int total = __shfl(incl, 63, 64);
        M.incl[lane] = incl;
        M.p0[lane] = p0;
        M.fa[lane] = 0;
        M.fb[lane] = 0;
        gb_wave_sync();
        if (total > 0) {
            const int c = (total + 63) >> 6;
            const int s0 = lane * c;
            const int e1 = s0 + c < total ? s0 + c : total;
            if (s0 < e1) {
                int row = 0;  // first row with incl > s0
#pragma unroll
                for (int st = 32; st > 0; st >>= 1)
                    if (M.incl[row + st - 1] <= s0) row += st;
                int rbeg = row ? M.incl[row - 1] : 0, rend = M.incl[row];
                bool before = rbeg < s0;
                int64_t pbase = M.p0[row] - rbeg;
                bool f = false;
                Z z = Z();
                for (int e = s0; e < e1; e += 4) {
                    int rw[4];
                    int64_t pos[4];
                    bool ok[4];
                    // positions of the next four entries (row changes from LDS)
                    int trow = row, tbeg = rbeg, tend = rend;
                    int64_t tbase = pbase;
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int et = e + t;
                        ok[t] = et < e1;
                        if (ok[t]) {
                            while (et >= tend) {
                                trow++;
                                tbeg = tend;
                                tend = M.incl[trow];
                                tbase = M.p0[trow] - tbeg;
                            }
                        }
                        rw[t] = trow;
                        pos[t] = tbase + et;
                    }
                    int k[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) k[t] = ok[t] ? colidx[pos[t]] : 0;
                    bool hit[4];
                    Z zt[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        hit[t] = ok[t] && (ufull || gb_bit(ubits, k[t]));
                        zt[t] = Z();
                        if (hit[t])
                            gb_spmv_product<SR, X, Z, FLIP>(sr, rv, avals, a_iso, a0, uvals, u_iso, u0, pos[t], k[t],
                                                            (w << 6) + rw[t], zt[t], uhot);
                    }
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        if (!ok[t]) break;
                        if (rw[t] != row) {  // the current row closed inside this run
                            if (before) {
                                M.pa[lane] = z;
                                M.fa[lane] = f;
                            } else if (f) {
                                acc[row] = z;
                                fl[row] = 1;
                            }
                            row = rw[t];
                            before = false;
                            f = false;
                        }
                        if (hit[t]) {
                            z = f ? sr.add(z, zt[t]) : zt[t];
                            f = true;
                        }
                    }
                    row = trow;
                    rbeg = tbeg;
                    rend = tend;
                    pbase = tbase;
                }
                // the row open at the end of the run
                const bool cont = rend > e1;
                if (before) {
                    M.pa[lane] = z;
                    M.fa[lane] = f;
                } else if (cont) {
                    M.pb[lane] = z;
                    M.fb[lane] = f;
                } else if (f) {
                    acc[row] = z;
                    fl[row] = 1;
                }
            }
            gb_wave_sync();
            // rows crossing runs: the owner lane folds the carries in lane order
            if (len > 0) {
                const int ex = incl - len;
                const int k0 = ex / c, k1 = (incl - 1) / c;
                if (k1 > k0) {
                    bool f = M.fb[k0] != 0;
                    Z z = M.pb[k0];
                    for (int k = k0 + 1; k <= k1; k++) {
                        if (!M.fa[k]) continue;
                        z = f ? sr.add(z, M.pa[k]) : M.pa[k];
                        f = true;
                    }
                    if (f) {
                        acc[lane] = z;
                        fl[lane] = 1;
                    }
                }
            }
            gb_wave_sync();
        }
        const bool hitrow = fl[lane] != 0;
        const unsigned long long fmask = __ballot(hitrow);
        if (hitrow) tvals[r] = acc[lane];
        if (lane == 0) {
            tbits[w] = fmask;
            cnt += __popcll(fmask);
        }
        fl[lane] = 0;
        gb_wave_sync();
    }
    return cnt;
}

template <class SR, class X, class Z, bool FLIP>
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_words(
    SR sr, int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    const X *__restrict__ avals, bool a_iso, const uint64_t *__restrict__ ubits,
    const X *__restrict__ uvals, bool u_iso, const uint64_t *__restrict__ mbits, bool mcomp,
    const int32_t *__restrict__ chunks, int64_t nchunks, Z *__restrict__ cpart, int8_t *__restrict__ cfound,
    uint64_t *__restrict__ tbits, Z *__restrict__ tvals, unsigned long long *__restrict__ tcount,
    unsigned long long *__restrict__ gst, const int64_t *__restrict__ ucount, int64_t un, int mode,
    const X *__restrict__ uhot) {
    __shared__ Z accs[WAVES_PER_BLOCK][64];
    __shared__ int fls[WAVES_PER_BLOCK][64];
    __shared__ gb_mp_lds<Z> mps[WAVES_PER_BLOCK];
    Z *acc = accs[threadIdx.x >> 6];
    int *fl = fls[threadIdx.x >> 6];  // row has at least one product
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nwords = (nrows + 63) >> 6;
    const bool rv = SR::reads_values && avals && uvals;
    X a0 = X(), u0 = X();
    if (rv) {
        if (a_iso) a0 = avals[0];
        if (u_iso) u0 = uvals[0];
    }
    // u has every entry: no presence tests (a relabelled colidx, uhot, is used only then)
    const bool ufull = uhot || (ucount && *ucount == un);
    const bool nt = (mode & 2) != 0;  // non-temporal loads of the streamed colidx / values
    mode &= 1;
    fl[lane] = 0;
    gb_wave_sync();
    long long cnt = 0;
    // long-row chunks: lane-sequential folds in ascending k, then a wave fold in lane order
    for (int64_t c = wave; c < nchunks; c += nwaves) {
        const int64_t r = chunks[2 * c], piece = chunks[2 * c + 1];
        bool f = false;
        Z z = Z();
        if (!mbits || gb_bit(mbits, r) != mcomp) {
            const int64_t pe = rowptr[r + 1];
            const int64_t p0 = rowptr[r] + piece * SPMV_CH;
            const int64_t p1 = p0 + SPMV_CH < pe ? p0 + SPMV_CH : pe;
            for (int64_t q = p0 + lane; q < p1; q += 256) {
                int kk[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    ok[u] = q + 64 * u < p1;
                    kk[u] = ok[u] ? (nt ? __builtin_nontemporal_load(&colidx[q + 64 * u]) : colidx[q + 64 * u]) : 0;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!ok[u] || (!ufull && !gb_bit(ubits, kk[u]))) continue;
                    Z t;
                    gb_spmv_product<SR, X, Z, FLIP>(sr, rv, avals, a_iso, a0, uvals, u_iso, u0, q + 64 * u, kk[u],
                                                    r, t, uhot, nt);
                    z = f ? sr.add(z, t) : t;
                    f = true;
                }
            }
        }
        for (int off = 1; off < 64; off <<= 1) {  // fold lanes in order: lane l absorbs l+off
            const bool of = __shfl_down((int)f, off, 64);
            const Z oz = gb_shfl_down(z, off, 64);
            if (lane + off < 64 && (lane & (2 * off - 1)) == 0 && of) {
                z = f ? sr.add(z, oz) : oz;
                f = true;
            }
        }
        if (lane == 0) {
            cfound[c] = f ? 1 : 0;
            if (f) cpart[c] = z;
        }
    }
    // output words
    if (mode == 1) {
        cnt += gb_spmv_words_mp<SR, X, Z, FLIP>(sr, nrows, rowptr, colidx, avals, a_iso, a0, ubits, uvals, u_iso, u0,
                                                mbits, mcomp, ufull, rv, tbits, tvals, acc, fl, mps[threadIdx.x >> 6],
                                                uhot);
        long long tot;
        if (gb_grid_sum(cnt, gst, &tot)) *tcount = (unsigned long long)tot;
        return;
    }
    for (int64_t w = wave; w < nwords; w += nwaves) {
        const int64_t r = (w << 6) + lane;
        bool open = r < nrows;
        if (open && mbits) open = gb_bit(mbits, r) != mcomp;
        int64_t p0 = 0;
        int len = 0;
        if (open) {
            p0 = rowptr[r];
            const int64_t d = rowptr[r + 1] - p0;
            len = d > SPMV_LONG ? 0 : (int)d;  // long rows: chunks + k_spmv_fold
        }
        int incl = len;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        const int excl = incl - len;
        const int total = __shfl(incl, 63, 64);
        for (int e0 = 0; e0 < total; e0 += 64 * SPMV_WU) {
            // all SPMV_WU gathers of the step are issued before the first fold waits on one
            int k[SPMV_WU], own[SPMV_WU];
            int64_t pos[SPMV_WU];
            bool ok[SPMV_WU];
#pragma unroll
            for (int u = 0; u < SPMV_WU; u++) {
                const int e = e0 + lane + 64 * u;
                int lo = 0;
#pragma unroll
                for (int st = 32; st > 0; st >>= 1)
                    if (__shfl(incl, lo + st - 1, 64) <= e) lo += st;
                own[u] = lo;
                pos[u] = __shfl(p0, lo, 64) + (e - __shfl(excl, lo, 64));
                ok[u] = e < total;
                k[u] = ok[u] ? (nt ? __builtin_nontemporal_load(&colidx[pos[u]]) : colidx[pos[u]]) : 0;
            }
            bool fu[SPMV_WU];
            Z zu[SPMV_WU];
#pragma unroll
            for (int u = 0; u < SPMV_WU; u++) {
                fu[u] = ok[u] && (ufull || gb_bit(ubits, k[u]));
                zu[u] = Z();
                if (fu[u])
                    gb_spmv_product<SR, X, Z, FLIP>(sr, rv, avals, a_iso, a0, uvals, u_iso, u0, pos[u], k[u],
                                                    (w << 6) + own[u], zu[u], uhot, nt);
            }
#pragma unroll
            for (int u = 0; u < SPMV_WU; u++) {
                bool f = fu[u];
                Z z = zu[u];
                // segmented inclusive scan over lanes of the same row; the segments and the
                // products' presence travel as two ballots, so each step shuffles only z:
                // before step off, lane l holds [max(seg, l-off+1), l]
                const int row = ok[u] ? own[u] : 64 + lane;  // idle lanes: own segment
                const int prow = __shfl_up(row, 1, 64);  // all lanes shuffle (not under ||)
                const unsigned long long heads = __ballot(lane == 0 || prow != row);
                const unsigned long long fmask = __ballot(f);
                const int seg = 63 - __clzll(heads & ((2ULL << lane) - 1ULL));  // this row's first lane
                for (int off = 1; off < 64; off <<= 1) {
                    const Z oz = gb_shfl_up(z, off, 64);
                    const int hi = lane - off;
                    if (hi >= seg) {
                        const int lo = hi - off + 1 > seg ? hi - off + 1 : seg;
                        if ((fmask >> lo) & ((2ULL << (hi - lo)) - 1ULL)) {  // lane hi's range holds a product
                            z = f ? sr.add(oz, z) : oz;
                            f = true;
                        }
                    }
                }
                const bool last = ok[u] && (lane == 63 || ((heads >> (lane + 1)) & 1ULL));
                // a row's runs arrive in order (earlier batches first): fold into its accumulator
                if (last && f) {
                    acc[row] = fl[row] ? sr.add(acc[row], z) : z;
                    fl[row] = 1;
                }
                gb_wave_sync();
            }
        }
        const bool hit = fl[lane] != 0;
        const unsigned long long fmask = __ballot(hit);
        if (hit) tvals[r] = acc[lane];
        if (lane == 0) {
            tbits[w] = fmask;
            cnt += __popcll(fmask);
        }
        fl[lane] = 0;
        gb_wave_sync();
    }
    long long tot;
    if (gb_grid_sum(cnt, gst, &tot)) *tcount = (unsigned long long)tot;  // k_spmv_fold adds the long rows
}

// the hot columns' values of a dense u, packed in rank order (gb_view_hot)
template <class X>
__global__ void k_hot_gather(const X *__restrict__ uvals, const int32_t *__restrict__ hcols, int64_t nh,
                             X *__restrict__ uhot) {
    for (int64_t h = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; h < nh; h += (int64_t)gridDim.x * blockDim.x)
        uhot[h] = uvals[hcols[h]];
}

// long rows: fold their chunks' partials in chunk order (one thread per row)
template <class SR, class Z>
__global__ void k_spmv_fold(SR sr, const int32_t *__restrict__ chunks, int64_t nchunks, const Z *__restrict__ cpart,
                            const int8_t *__restrict__ cfound, uint64_t *__restrict__ tbits, Z *__restrict__ tvals,
                            unsigned long long *__restrict__ tcount, unsigned long long *__restrict__ gst) {
    long long cnt = 0;
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nchunks;
         c += (int64_t)gridDim.x * blockDim.x) {
        if (chunks[2 * c + 1] != 0) continue;
        const int64_t r = chunks[2 * c];
        bool f = false;
        Z z = Z();
        for (int64_t h = c; h < nchunks && chunks[2 * h] == r; h++) {
            if (!cfound[h]) continue;
            z = f ? sr.add(z, cpart[h]) : cpart[h];
            f = true;
        }
        if (f) {
            tvals[r] = z;
            atomicOr((unsigned long long *)&tbits[r >> 6], 1ULL << (r & 63));
            cnt++;
        }
    }
    gb_grid_add(cnt, tcount, gst);
}

// hub-chunk table of a CSR: pieces per row, then (row, piece) pairs
__global__ void k_hub_count(const int64_t *__restrict__ rowptr, int64_t n, int64_t thresh, int64_t H,
                            int64_t *__restrict__ cnt) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = rowptr[r + 1] - rowptr[r];
        cnt[r] = d > thresh ? (d + H - 1) / H : 0;
    }
}
// rec (nullptr: not kept): a record per piece -- row, entry count, first entry position
__global__ void k_hub_fill(const int64_t *__restrict__ cnt, const int64_t *__restrict__ off, int64_t n,
                           int32_t *__restrict__ tab, const int64_t *__restrict__ rowptr, int64_t H,
                           gb_hub_piece *__restrict__ rec) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = cnt[r], o = off[r];
        for (int64_t i = 0; i < c; i++) {
            tab[2 * (o + i)] = (int32_t)r;
            tab[2 * (o + i) + 1] = (int32_t)i;
            if (rec) {
                const int64_t p0 = rowptr[r] + i * H, left = rowptr[r + 1] - p0;
                rec[o + i] = gb_hub_piece{(int32_t)r, (int32_t)(left < H ? left : H), p0};
            }
        }
    }
}
__global__ void k_row_len_u32(const int64_t *__restrict__ rowptr, int64_t n, uint32_t *__restrict__ out) {
    GB_GRID_LOOP(r, n)
        out[r] = (uint32_t)(rowptr[r + 1] - rowptr[r]);
}

// (row, piece) table of the rows of v longer than thresh, cut into H-entry pieces.  sections:
// the allocation goes on after the pairs with a record per piece and every row's length
// (gb_hub_sections_of, gb_internal.h) -- the hub table of the BFS push
static int32_t *gb_build_chunk_table(const gb_csr_view &v, int64_t thresh, int64_t H, int64_t *total_out,
                                     bool sections = false) {
    const int64_t n = v.nrows;
    gb_scratch s;
    int64_t *cnt = s.get<int64_t>(n + 1);
    int64_t *off = s.get<int64_t>(n + 1);
    const unsigned g = gb_grid(n, 256, 8192);
    hipLaunchKernelGGL(k_hub_count, dim3(g), dim3(256), 0, gb_stream(), v.rowptr, n, thresh, H, cnt);
    GB_LAUNCH_CHECK();
    gb_exclusive_scan_i64(cnt, off, n);
    const int64_t total = gb_read_i64(off + n);
    int32_t *tab = gb_malloc_n<int32_t>(sections ? gb_hub_table_ints(total, n) : 2 * total + 2);
    const gb_hub_sections sec = sections ? gb_hub_sections_of(tab, total) : gb_hub_sections{};
    hipLaunchKernelGGL(k_hub_fill, dim3(g), dim3(256), 0, gb_stream(), cnt, off, n, tab, v.rowptr, H,
                       const_cast<gb_hub_piece *>(sec.piece));
    GB_LAUNCH_CHECK();
    if (sections) {
        hipLaunchKernelGGL(k_row_len_u32, dim3(g), dim3(256), 0, gb_stream(), v.rowptr, n,
                           const_cast<uint32_t *>(sec.rowlen));
        GB_LAUNCH_CHECK();
    }
    *total_out = total;
    return tab;
}

__global__ void k_row_maxlen(const int64_t *__restrict__ rowptr, int64_t n, unsigned long long *__restrict__ mx) {
    unsigned long long m = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long d = (unsigned long long)(rowptr[r + 1] - rowptr[r]);
        m = d > m ? d : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(mx, m);
}

void gb_view_hubs(gb_csr_view &v, GB_Obj *A, int orient, int64_t H) {
    if (A->kind != GB_KIND_MATRIX) return;
    gb_orient_cache &c = A->oc[orient];
    if (!c.hub_tab || c.hub_H != H) {
        gb_stat_add("hub_tables_built", 1);
        gb_free(c.hub_tab);
        c.hub_tab = gb_build_chunk_table(v, H, H, &c.hub_n, true);
        c.hub_H = H;
        // the longest row, for host-side direction decisions on small frontiers (gb_spmv_iso)
        gb_scratch s;
        unsigned long long *mx = s.get<unsigned long long>(1);
        gb_memset(mx, 0, sizeof(unsigned long long));
        const unsigned g = gb_grid(v.nrows, 256, 2048);
        hipLaunchKernelGGL(k_row_maxlen, dim3(g), dim3(256), 0, gb_stream(), v.rowptr, v.nrows, mx);
        GB_LAUNCH_CHECK();
        unsigned long long h = 0;
        gb_copy_d2h(&h, mx, sizeof(h));
        c.maxdeg = (int64_t)h;
    }
    v.hubs = c.hub_tab;
    v.nhubs = c.hub_n;
    v.hub_H = H;
    v.maxdeg = c.maxdeg;
}

void gb_view_long_rows(gb_csr_view &v, GB_Obj *A, int orient) {
    if (A->kind != GB_KIND_MATRIX) return;
    gb_orient_cache &c = A->oc[orient];
    if (!c.long_tab) {
        gb_stat_add("long_tables_built", 1);
        c.long_tab = gb_build_chunk_table(v, SPMV_LONG, SPMV_CH, &c.long_n);
    }
    v.lchunks = c.long_tab;
    v.nlchunks = c.long_n;
}

// ne[w]: bitmap word of the rows with entries (bits past n clear); pc[w]: its popcount
__global__ void k_rows_nonempty(const int64_t *__restrict__ rowptr, int64_t n, uint64_t *__restrict__ ne,
                                int32_t *__restrict__ pc) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (n + 63) >> 6;
    for (int64_t w = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; w < nw;
         w += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t r = (w << 6) + lane;
        const unsigned long long b = __ballot(r < n && rowptr[r + 1] > rowptr[r]);
        if (lane == 0) {
            ne[w] = b;
            pc[w] = __popcll(b);
        }
    }
}

__global__ void k_narrow_u32(const int64_t *__restrict__ in, uint32_t *__restrict__ out, int64_t n) {
    GB_GRID_LOOP(i, n)
        out[i] = (uint32_t)in[i];
}

// the bitmap and, with it, its per-word exclusive prefix ne_rank (words + 1 entries, the last
// one the count of non-empty rows): the words' popcounts through the scan of gb_prim.hip
void gb_view_nonempty(gb_csr_view &v, GB_Obj *A, int orient) {
    if (A->kind != GB_KIND_MATRIX) return;
    gb_orient_cache &c = A->oc[orient];
    if (!c.rows_ne) {
        gb_stat_add("nonempty_built", 1);
        const int64_t nw = gb_words(v.nrows);
        c.rows_ne = gb_malloc_n<uint64_t>(nw);
        c.ne_rank = gb_malloc_n<uint32_t>(nw + 1);
        if (nw == 0) {
            gb_memset(c.ne_rank, 0, sizeof(uint32_t));
        } else {
            gb_scratch s;
            int32_t *pc = s.get<int32_t>(nw);
            int64_t *pre = s.get<int64_t>(nw + 1);
            const unsigned g = gb_grid(nw, 4, 8192);  // a wave per word
            hipLaunchKernelGGL(k_rows_nonempty, dim3(g), dim3(256), 0, gb_stream(), v.rowptr, v.nrows, c.rows_ne, pc);
            GB_LAUNCH_CHECK();
            gb_exclusive_scan_i32(pc, 0, pre, nw);
            hipLaunchKernelGGL(k_narrow_u32, dim3(gb_grid(nw + 1, 256, 4096)), dim3(256), 0, gb_stream(), pre,
                               c.ne_rank, nw + 1);
            GB_LAUNCH_CHECK();
        }
    }
    v.nonempty = c.rows_ne;
    v.ne_rank = c.ne_rank;
}

// pull heads: a wave per row picks its neighbours with the longest rows in the other
// orientation (ties: the smaller index) -- in a level BFS those are the ones most likely to
// be in the frontier, so most rows the pull settles are settled by them -- 3 of them for a
// row longer than 4 (4th slot -2: "walk the row"), the whole row otherwise (padding -1), and
// stores the row's own length in the other orientation (the next-frontier hint of a row
// settled without reading its bounds)
__device__ __forceinline__ void pf_better(int64_t &bd, int32_t &bi, int64_t d, int32_t i) {
    if (i >= 0 && (d > bd || (d == bd && (bi < 0 || i < bi)))) {
        bd = d;
        bi = i;
    }
}
// The records are indexed by the row's rank among the non-empty rows (ne: their bitmap, rank:
// its per-word exclusive prefix, gb_view_nonempty); a row without entries has none.
__global__ __launch_bounds__(256) void k_pull_head(int64_t n, const int64_t *__restrict__ rp,
                                                   const int32_t *__restrict__ ci,
                                                   const int64_t *__restrict__ orp, int64_t on,
                                                   const uint64_t *__restrict__ ne, const uint32_t *__restrict__ rank,
                                                   int4 *__restrict__ head, uint32_t *__restrict__ pdeg) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t j = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; j < n; j += nwaves) {
        const int64_t e0 = rp[j], e1 = rp[j + 1], d = e1 - e0;
        if (d <= 0) continue;  // the wave's row is empty: no record
        const int64_t slot = (int64_t)rank[j >> 6] + __popcll(ne[j >> 6] & ((1ULL << (j & 63)) - 1));
        int32_t pick[4] = {-1, -1, -1, -1};
        const int rounds = d <= 4 ? (int)d : 3;
        for (int r = 0; r < rounds; r++) {
            int64_t bd = -1;
            int32_t bi = -1;
            for (int64_t e = e0 + lane; e < e1; e += 64) {
                const int32_t i = ci[e];
                bool taken = false;
                for (int q = 0; q < r; q++) taken = taken || pick[q] == i;
                if (!taken) pf_better(bd, bi, orp[i + 1] - orp[i], i);
            }
            for (int off = 32; off > 0; off >>= 1) {
                const int64_t od = __shfl_xor(bd, off, 64);
                const int32_t oi = __shfl_xor(bi, off, 64);
                pf_better(bd, bi, od, oi);
            }
            pick[r] = bi;  // identical on every lane
        }
        if (d > 4) pick[3] = -2;
        if (lane == 0) {
            head[slot] = make_int4(pick[0], pick[1], pick[2], pick[3]);
            if (pdeg) {
                const int64_t od = j < on ? orp[j + 1] - orp[j] : 0;
                pdeg[slot] = (uint32_t)(od < 0xFFFFFFFFLL ? od : 0xFFFFFFFFLL);
            }
        }
    }
}

void gb_view_pullfirst(gb_csr_view &v, GB_Obj *A, int orient, const int64_t *other_rowptr, int64_t other_n) {
    if (A->kind != GB_KIND_MATRIX || v.nrows == 0) return;
    gb_orient_cache &c = A->oc[orient];
    // the records are found through the non-empty bitmap's ranks: no heads without them
    if (!c.rows_ne || !c.ne_rank || v.nonempty != c.rows_ne || v.ne_rank != c.ne_rank) return;
    if (!c.phead) {
        gb_stat_add("pull_heads_built", 1);
        // one record per non-empty row: their count is the prefix's last entry (read once per
        // matrix orientation, when the heads are built)
        uint32_t ne_count = 0;
        gb_copy_d2h(&ne_count, c.ne_rank + gb_words(v.nrows), sizeof(ne_count));
        const int64_t nrec = std::max<int64_t>(1, (int64_t)ne_count);
        c.phead = gb_malloc_n<int32_t>(4 * nrec);
        c.pdeg = gb_malloc_n<uint32_t>(nrec);
        const unsigned g = gb_grid(v.nrows, 4, 65535);  // a wave per row
        hipLaunchKernelGGL(k_pull_head, dim3(g), dim3(256), 0, gb_stream(), v.nrows, v.rowptr, v.colidx,
                           other_rowptr, other_n, c.rows_ne, c.ne_rank, reinterpret_cast<int4 *>(c.phead), c.pdeg);
        GB_LAUNCH_CHECK();
    }
    v.phead = c.phead;
    v.pdeg = c.pdeg;
}

static bool idempotent_monoid(int m) {
    return m == GBAMD_MON_ANY || m == GBAMD_MON_MIN || m == GBAMD_MON_MAX || m == GBAMD_MON_LOR ||
           m == GBAMD_MON_LAND || m == GBAMD_MON_BOR || m == GBAMD_MON_BAND;
}

bool gb_spmv_result_iso(GrB_Semiring sr, bool a_iso, bool u_iso, bool flip) {
    gb_sr_info info = gb_sr_describe(sr);
    bool reads_a = info.reads_values, reads_u = info.reads_values;
    if (info.mul == GBAMD_OP_FIRST) (flip ? reads_a : reads_u) = false;
    if (info.mul == GBAMD_OP_SECOND) (flip ? reads_u : reads_a) = false;
    if (info.mul == GBAMD_OP_PAIR) return idempotent_monoid(info.mon);
    return !info.positional && idempotent_monoid(info.mon) && (!reads_a || a_iso) && (!reads_u || u_iso);
}

// the runtime flip as a compile-time constant: f(std::bool_constant<flip>{}), so a launch's
// argument list is written once for both kernel instantiations
template <class F>
static void gb_with_flip(bool flip, F &&f) {
    if (flip) f(std::true_type{});
    else f(std::false_type{});
}

void gb_spmv(gb_vec_result &T, const gb_csr_view &A, const gb_csr_view *Apush, gb_bitmap_view &u,
             const gb_vmask &mask, GrB_Semiring sr, bool flip, const gb_asg *asg) {
    gb_sr_info info = gb_sr_describe(sr);
    gb_scratch s;
    gb_csr_view &Av = const_cast<gb_csr_view &>(A);
    const void *av = info.reads_values ? gb_view_vals_as(Av, info.xcode, s) : nullptr;
    const void *uv = info.reads_values ? gb_bitmap_vals_as(u, info.xcode, s) : nullptr;
    const bool iso = gb_spmv_result_iso(sr, A.iso, u.iso, flip);

    const int64_t n = A.nrows;
    const size_t zs = gb_type_size(info.zcode);
    T.n = n;
    T.tcode = info.zcode;
    T.iso = iso;
    T.bits = gb_malloc_n<uint64_t>(gb_words(n));
    T.dense = gb_malloc((iso ? 1 : n) * zs);
    // [0] count; [2 .. 2 + GB_HINT_PARTS): next-frontier edge hint in parts (iso path)
    T.d_nvals = gb_malloc_n<int64_t>(2 + GB_HINT_PARTS);
    if (n == 0) {
        gb_memset(T.d_nvals, 0, sizeof(int64_t));
        return;
    }

    if (iso) {  // the BFS path: not a template, no dispatch
        gb_spmv_iso(T, A, Apush, u, mask, sr, flip, asg, av, uv);
        return;
    }
    const int64_t nw = gb_words(n);
    unsigned long long *gst = gb_device_state();

    gb_dispatch_sr(info, [&](auto srf, auto x, auto z) {
        using SRT = decltype(srf);
        using X = decltype(x);
        using Z = decltype(z);
        if (A.nlchunks >= 0 && gb_knob("spmv_general") != 1) {
            // general semiring: balanced words + long-row chunks (+ their fold)
            Z *cpart = s.get<Z>(A.nlchunks + 1);
            int8_t *cfound = s.get<int8_t>(A.nlchunks + 1);
            const int64_t units = std::max<int64_t>(nw, A.nlchunks);
            const bool u_iso_k = u.iso || gb_knob("spmv_timing_no_x_gather") == 1;  // timing experiment only
            int spmv_mode = gb_knob("spmv_words") == 2 ? 1 : 0;  // 0: segmented scan (default), 2: merge path
            if (gb_knob("spmv_nt") == 1) spmv_mode |= 2;
            const unsigned grid = gb_grid(units, SPMV_BLOCK / 64, 4096);
            // dense u on a relabelled matrix: the hot columns' values packed first (gb_view_hot);
            // positional multipliers need the true column, so they keep the plain colidx
            const int32_t *ci = A.colidx;
            X *uhot = nullptr;
            if (A.hcolidx && u.full && !u_iso_k && uv && !info.positional && info.reads_values) {
                uhot = s.get<X>(A.nhot);
                const unsigned hg = gb_grid(A.nhot, 256, 2048);
                hipLaunchKernelGGL((k_hot_gather<X>), dim3(hg), dim3(256), 0, gb_stream(), (const X *)uv, A.hcols,
                                   A.nhot, uhot);
                GB_LAUNCH_CHECK();
                ci = A.hcolidx;
            }
            gb_with_flip(flip, [&](auto fl) {
                hipLaunchKernelGGL((k_spmv_words<SRT, X, Z, decltype(fl)::value>), dim3(grid), dim3(SPMV_BLOCK), 0,
                                   gb_stream(), srf, n, A.rowptr, ci, (const X *)av, A.iso, u.bits, (const X *)uv,
                                   u_iso_k, mask.bits, mask.comp, A.lchunks, A.nlchunks, cpart, cfound, T.bits,
                                   (Z *)T.dense, (unsigned long long *)T.d_nvals, gst, u.count, u.n, spmv_mode,
                                   (const X *)uhot);
            });
            GB_LAUNCH_CHECK();
            if (A.nlchunks > 0) {
                const unsigned fg = gb_grid(A.nlchunks, 256, 1024);
                hipLaunchKernelGGL((k_spmv_fold<SRT, Z>), dim3(fg), dim3(256), 0, gb_stream(), srf, A.lchunks,
                                   A.nlchunks, cpart, cfound, T.bits, (Z *)T.dense, (unsigned long long *)T.d_nvals,
                                   gst);
                GB_LAUNCH_CHECK();
            }
            return;
        }
        // fallback (no long-row table: the operand is not a matrix object): G lanes per row
        gb_memset(T.d_nvals, 0, sizeof(int64_t));
        const int64_t avg = (A.nvals + n - 1) / n;
        int lg = 0;
        while (lg < 6 && (1LL << lg) < avg) lg++;
        const int64_t forced = gb_knob("spmv_lg");
        if (forced > 0) lg = (int)(forced - 1);
        const unsigned grid = gb_grid(n, SPMV_TILE, 2048);  // n > 0 here
        gb_with_flip(flip, [&](auto fl) {
            hipLaunchKernelGGL((k_spmv_pull<SRT, X, Z, decltype(fl)::value>), dim3(grid), dim3(SPMV_BLOCK), 0,
                               gb_stream(), srf, n, A.rowptr, A.colidx, (const X *)av, A.iso, u.bits, (const X *)uv,
                               u.iso, mask.bits, mask.comp, lg, T.bits, (Z *)T.dense,
                               (unsigned long long *)T.d_nvals, gst);
        });
        GB_LAUNCH_CHECK();
    });
}
