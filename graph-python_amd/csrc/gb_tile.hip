// gb_tile.hip -- GxB_Matrix_concat / GxB_Matrix_split: a matrix from m x n tiles, and back.
//   reference core/ss/matrix.py:281-381, core/ss/vector.py:185-265, ss/_core.py:73-107
// Tiles is row-major (tile (i, j) = Tiles[i * n + j]); no mask, no accumulator.  Both are
// entry-parallel (a hub row of an R-MAT graph costs per entry what a row of 3 does), without
// atomics, columns ascending, the same bits every run, and their launches do not grow with m * n.
//
// Matrix concat.  rb[i] = the first output row of tile-row i, ebase[i] = the entries of the
// tile-rows above it (CSR nvals are host-known), coff[j] = the first output column of tile-column
// j.  One table of tile records goes to the device (the call's one upload; nothing is read back
// unless every tile with entries is iso, see below):
//   k_concat_rowptr  output row r = rb[i] + l: crp[r] = ebase[i] + sum_j rp_ij[l]; the same lane
//                    leaves start_ij[l] = crp[r] + (entries of row l in the tiles left of j)
//                    - rp_ij[l] for every tile of its tile-row, so that
//   k_concat_fill    entry p of tile (i, j), local row l (the wave row search of gb_chunk_rows,
//                    over chunks of 256 entries numbered through all tiles), lands at
//                    start_ij[l] + p with column ci[p] + coff[j] and its value cast to C's type:
//                    one load for the position however many tile columns there are.  With one
//                    tile column (row panels) a tile's entries stay together: entry p lands at
//                    (the entries of the tiles before) + p, no row search and no start array
// The result is iso only when every tile with entries is iso and their values, cast to C's type,
// have equal bits: with one such tile that is known at once, with more k_tile_iso_gather casts
// the values into one array and the host reads it (8 bytes per tile).
//
// Matrix split.  cb[j] = the first column of tile-column j.  The counts of all tiles sit in one
// layout, tile-major, tile t = (i, j) at loff[t] with nrows_i + 1 slots (the last one zero):
//   k_split_count    slot (t, l): row rb[i] + l of A is cut at cb[j] and cb[j + 1] by binary
//                    search; cnt = the entries between, cut = where they start
//   gb_exclusive_scan_i32 over the whole layout: S.  Tile t's row pointer is S[loff[t] + l]
//                    - S[loff[t]], its last element the tile's nvals
//   k_split_rowptr   writes every tile's row pointer and total, and turns cut into
//                    delta = rowptr_t[l] - cut, so that
//   (one read of the m * n totals sizes the tiles' columns and values)
//   k_split_fill     entry p of A (row r by the wave row search, column c): tile-row by a search
//                    of rb, tile-column by a search of cb, lands at p + delta in its tile with
//                    column c - cb[j]; an iso A writes its one value where it lands first
// Work and memory are O(nvals + nrows * n + m * n), what the tiles' row pointers take anyway.
//
// Vectors stay bitmaps: k_tile_bits moves bits [s, s + len) of one bitmap to bit d of another,
// one destination word per lane from at most two source words; the dense values move as
// contiguous ranges (gb_cast_array when the types differ).  One launch per piece.
//
// "stat_concat_bitmap" / "stat_split_bitmap": the last call moved bitmaps (1) or built CSR (0);
// "stat_concat_iso": the last concat's result was iso.
#include <algorithm>
#include <memory>
#include <vector>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define TILE_BLOCK 256
#define TILE_WPI 4  // words of 64 entries a wave handles per chunk
#define TILE_GRID_CAP 8192

namespace {

// one tile of a concat, as the device sees it
struct tile_rec {
    const int64_t *rp;
    const int32_t *ci;
    const void *vx;
    int64_t nrows, nvals;
    int64_t soff;   // this tile's part of the start array
    int64_t ebase;  // the entries of the tiles before it, row-major: where a row panel's entries go
    int32_t coff;   // first output column
    int32_t tcode;
    int32_t iso;
    int32_t pad;
};

// element idx of an array of runtime type `code`, cast to D
template <class D>
GB_DEV D tile_load(const void *__restrict__ vx, int code, int64_t idx) {
    switch (code) {
    case GBAMD_T_BOOL: return gb_cast<D, bool>(((const bool *)vx)[idx]);
    case GBAMD_T_INT8: return gb_cast<D, int8_t>(((const int8_t *)vx)[idx]);
    case GBAMD_T_UINT8: return gb_cast<D, uint8_t>(((const uint8_t *)vx)[idx]);
    case GBAMD_T_INT16: return gb_cast<D, int16_t>(((const int16_t *)vx)[idx]);
    case GBAMD_T_UINT16: return gb_cast<D, uint16_t>(((const uint16_t *)vx)[idx]);
    case GBAMD_T_INT32: return gb_cast<D, int32_t>(((const int32_t *)vx)[idx]);
    case GBAMD_T_UINT32: return gb_cast<D, uint32_t>(((const uint32_t *)vx)[idx]);
    case GBAMD_T_INT64: return gb_cast<D, int64_t>(((const int64_t *)vx)[idx]);
    case GBAMD_T_UINT64: return gb_cast<D, uint64_t>(((const uint64_t *)vx)[idx]);
    case GBAMD_T_FP32: return gb_cast<D, float>(((const float *)vx)[idx]);
    default: return gb_cast<D, double>(((const double *)vx)[idx]);
    }
}

// last index i in [0, count) with bound[i] <= x (bound[0] <= x < bound[count] is known): the
// part of a cut that holds x; equal neighbours (an empty part) are skipped
GB_DEV int64_t tile_part(const int64_t *__restrict__ bound, int64_t count, int64_t x) {
    return gb_upper_bound(bound, 1, count, x) - 1;
}

// ------------------------------------------------------------------ matrix concat
__global__ __launch_bounds__(TILE_BLOCK) void k_concat_rowptr(int64_t nrows, int64_t total, int64_t m, int64_t n,
                                                              const tile_rec *__restrict__ tiles,
                                                              const int64_t *__restrict__ rb,
                                                              const int64_t *__restrict__ ebase,
                                                              int64_t *__restrict__ crp,
                                                              int64_t *__restrict__ start) {
    GB_GRID_LOOP(r, nrows + 1) {
        if (r == nrows) {
            crp[r] = total;
            continue;
        }
        const int64_t i = tile_part(rb, m, r);
        const int64_t l = r - rb[i];
        const tile_rec *__restrict__ row = tiles + i * n;
        int64_t acc = ebase[i];
        for (int64_t j = 0; j < n; j++) acc += row[j].rp[l];
        crp[r] = acc;
        if (!start) continue;
        for (int64_t j = 0; j < n; j++) {
            const int64_t a = row[j].rp[l];
            start[row[j].soff + l] = acc - a;
            acc += row[j].rp[l + 1] - a;
        }
    }
}

// chunk g of the call belongs to tile t with cbase[t] <= g < cbase[t + 1]; a wave takes a run
// of chunks and restarts its row search where the tile changes.  VALS == false: iso result.
// PANELS: one tile column (row panels): a tile's entries stay together, entry p lands at
// ebase + p, and nobody needs its row
template <class D, bool VALS, bool PANELS>
__global__ __launch_bounds__(TILE_BLOCK) void k_concat_fill(int64_t nchunks, int64_t ntiles,
                                                            const tile_rec *__restrict__ tiles,
                                                            const int64_t *__restrict__ cbase,
                                                            const int64_t *__restrict__ start,
                                                            int32_t *__restrict__ oci, D *__restrict__ ox) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * TILE_BLOCK) >> 6;
    const int64_t per_wave = (nchunks + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)TILE_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, nchunks);
    int64_t t = -1, tend = 0, next = -1;
    for (int64_t g = g0; g < g1; g++) {
        if (g >= tend) {
            t = tile_part(cbase, ntiles, g);
            tend = cbase[t + 1];
            next = -1;
        }
        const tile_rec rec = tiles[t];
        const int64_t p0 = ((g - cbase[t]) * TILE_WPI) << 6;
        int64_t row[TILE_WPI];
        if (!PANELS) gb_chunk_rows<TILE_WPI>(rec.rp, rec.nrows, rec.nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < TILE_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= rec.nvals) continue;
            const int64_t dst = PANELS ? rec.ebase + p : start[rec.soff + row[u]] + p;
            oci[dst] = rec.ci[p] + rec.coff;
            if (VALS) ox[dst] = tile_load<D>(rec.vx, rec.tcode, rec.iso ? 0 : p);
        }
    }
}

// out[t] = the first value of tile t cast to D, in the low bytes of a zeroed word
template <class D>
__global__ void k_tile_iso_gather(int64_t ntiles, const tile_rec *__restrict__ tiles,
                                  unsigned long long *__restrict__ out) {
    GB_GRID_LOOP(t, ntiles) {
        unsigned long long w = 0;
        if (tiles[t].nvals > 0) {
            const D v = tile_load<D>(tiles[t].vx, tiles[t].tcode, 0);
            memcpy(&w, &v, sizeof(D));
        }
        out[t] = w;
    }
}

// ------------------------------------------------------------------ matrix split
// the layout's slot x belongs to tile t = tile_part(loff, x), local row l = x - loff[t]
__global__ __launch_bounds__(TILE_BLOCK) void k_split_count(int64_t nslots, int64_t ntiles, int64_t n,
                                                            const int64_t *__restrict__ rb,
                                                            const int64_t *__restrict__ cb,
                                                            const int64_t *__restrict__ loff,
                                                            const int64_t *__restrict__ arp,
                                                            const int32_t *__restrict__ aci,
                                                            int32_t *__restrict__ cnt, int64_t *__restrict__ cut) {
    GB_GRID_LOOP(x, nslots) {
        const int64_t t = tile_part(loff, ntiles, x);
        const int64_t i = t / n, j = t - i * n;
        const int64_t l = x - loff[t];
        int64_t a = 0, b = 0;
        if (l < rb[i + 1] - rb[i]) {
            const int64_t r = rb[i] + l;
            const int64_t lo = arp[r], hi = arp[r + 1];
            a = j == 0 ? lo : gb_lower_bound(aci, lo, hi, cb[j]);
            b = j == n - 1 ? hi : gb_lower_bound(aci, a, hi, cb[j + 1]);
        }
        cnt[x] = (int32_t)(b - a);
        cut[x] = a;
    }
}

// S: the exclusive scan of cnt.  trp[t]: tile t's row pointer; cut becomes delta in place
__global__ __launch_bounds__(TILE_BLOCK) void k_split_rowptr(int64_t nslots, int64_t ntiles,
                                                             const int64_t *__restrict__ loff,
                                                             const int64_t *__restrict__ S,
                                                             int64_t *const *__restrict__ trp,
                                                             int64_t *__restrict__ cut, int64_t *__restrict__ totals) {
    GB_GRID_LOOP(x, nslots) {
        const int64_t t = tile_part(loff, ntiles, x);
        const int64_t l = x - loff[t];
        const int64_t v = S[x] - S[loff[t]];
        trp[t][l] = v;
        cut[x] = v - cut[x];
        if (x + 1 == loff[t + 1]) totals[t] = v;
    }
}

// VS: bytes per value.  iso: A holds one value, and so does every tile with entries
template <int VS>
__global__ __launch_bounds__(TILE_BLOCK) void k_split_fill(int64_t nrows, int64_t nvals, int64_t m, int64_t n,
                                                           const int64_t *__restrict__ rb,
                                                           const int64_t *__restrict__ cb,
                                                           const int64_t *__restrict__ loff,
                                                           const int64_t *__restrict__ delta,
                                                           const int64_t *__restrict__ arp,
                                                           const int32_t *__restrict__ aci,
                                                           const void *__restrict__ avx_, bool iso,
                                                           int32_t *const *__restrict__ tci,
                                                           void *const *__restrict__ tvx) {
    using V = gb_word_t<VS>;
    const V *__restrict__ avx = (const V *)avx_;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * TILE_BLOCK) >> 6;
    const int64_t nchunks = (nvals + TILE_WPI * 64 - 1) / (TILE_WPI * 64);
    const int64_t per_wave = (nchunks + nwaves - 1) / nwaves;
    const int64_t g0 = ((blockIdx.x * (int64_t)TILE_BLOCK + threadIdx.x) >> 6) * per_wave;
    const int64_t g1 = min(g0 + per_wave, nchunks);
    int64_t next = -1;
    for (int64_t g = g0; g < g1; g++) {
        const int64_t p0 = (g * TILE_WPI) << 6;
        int64_t row[TILE_WPI];
        gb_chunk_rows<TILE_WPI>(arp, nrows, nvals, p0, lane, next, row);
#pragma unroll
        for (int u = 0; u < TILE_WPI; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p >= nvals) continue;
            const int64_t r = row[u];
            const int64_t c = aci[p];
            const int64_t i = tile_part(rb, m, r);
            const int64_t j = tile_part(cb, n, c);
            const int64_t t = i * n + j;
            const int64_t dst = p + delta[loff[t] + (r - rb[i])];
            tci[t][dst] = (int32_t)(c - cb[j]);
            if (!iso) ((V *)tvx[t])[dst] = avx[p];
            else if (dst == 0) ((V *)tvx[t])[0] = avx[0];
        }
    }
}

// ------------------------------------------------------------------ bitmaps
// Bits [s, s + len) of src (nsw words) go to bits [d, d + len) of dst, one lane per destination
// word w0 + k.  A word the range covers only partly keeps its other bits when merge is set (the
// pieces of a concat share words, launch after launch on one stream) and gets them zero otherwise
__global__ __launch_bounds__(TILE_BLOCK) void k_tile_bits(const uint64_t *__restrict__ src, int64_t nsw, int64_t s,
                                                          int64_t len, uint64_t *__restrict__ dst, int64_t d,
                                                          bool merge) {
    const int64_t w0 = d >> 6;
    const int64_t nw = ((d + len - 1) >> 6) - w0 + 1;
    GB_GRID_LOOP(k, nw) {
        const int64_t w = w0 + k;
        const int64_t b0 = max(w << 6, d), b1 = min((w + 1) << 6, d + len);  // destination bits [b0, b1)
        const int nb = (int)(b1 - b0);
        uint64_t mask = nb == 64 ? ~0ull : ((1ull << nb) - 1) << (b0 & 63);
        // the 64 source bits that line up with destination word w start at bit q (below 0 in the
        // first word when d is further into its word than s)
        const int64_t q = (w << 6) - d + s;
        const int64_t sw = q >> 6;  // floor
        const int sh = (int)(q & 63);
        const uint64_t lo = sw >= 0 && sw < nsw ? src[sw] : 0;
        uint64_t v = lo >> sh;
        if (sh) {
            const uint64_t hi = sw + 1 >= 0 && sw + 1 < nsw ? src[sw + 1] : 0;
            v |= hi << (64 - sh);
        }
        v &= mask;
        if (merge && nb != 64) v |= dst[w] & ~mask;
        dst[w] = v;
    }
}

// dst[d .. d + len) = *one
template <class W>
__global__ void k_tile_fill(W *__restrict__ dst, int64_t d, int64_t len, const W *__restrict__ one) {
    const W v = *one;
    GB_GRID_LOOP(k, len) dst[d + k] = v;
}

void tile_move_bits(const uint64_t *src, int64_t src_n, int64_t s, int64_t len, uint64_t *dst, int64_t d,
                    bool merge) {
    if (len <= 0) return;
    const int64_t nw = ((d + len - 1) >> 6) - (d >> 6) + 1;
    hipLaunchKernelGGL(k_tile_bits, dim3(gb_grid(nw, TILE_BLOCK, TILE_GRID_CAP)), dim3(TILE_BLOCK), 0, gb_stream(),
                       src, gb_words(src_n), s, len, dst, d, merge);
    GB_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ host side
struct tile_dims {
    int64_t m = 0, n = 0;
    std::vector<int64_t> rb, cb;  // m + 1 row bounds, n + 1 column bounds
};

// bounds from per-part sizes, checked against the whole
void tile_bounds(std::vector<int64_t> &bound, const std::vector<int64_t> &sizes, int64_t whole, const char *what) {
    bound.assign(sizes.size() + 1, 0);
    for (size_t k = 0; k < sizes.size(); k++) {
        GB_REQUIRE(sizes[k] >= 0 && sizes[k] <= whole - bound[k], GrB_DIMENSION_MISMATCH, what);
        bound[k + 1] = bound[k] + sizes[k];
    }
    GB_REQUIRE(bound.back() == whole, GrB_DIMENSION_MISMATCH, what);
}

// a device copy of several host arrays of int64-sized items, one upload; off[k] = where array k starts
struct tile_upload {
    std::vector<int64_t> host;
    std::vector<size_t> off;
    size_t add(const void *p, size_t bytes) {
        const size_t words = (bytes + 7) / 8, at = host.size();
        host.resize(at + words);
        if (bytes) memcpy(host.data() + at, p, bytes);
        off.push_back(at);
        return at;
    }
    int64_t *send(gb_scratch &s) {
        int64_t *d = s.get<int64_t>(host.size());
        gb_copy_h2d(d, host.data(), host.size() * sizeof(int64_t));
        return d;
    }
};

bool tile_values_equal(const std::vector<unsigned long long> &w, const std::vector<int64_t> &nv) {
    int64_t first = -1;
    for (size_t t = 0; t < w.size(); t++) {
        if (nv[t] <= 0) continue;
        if (first < 0) first = (int64_t)t;
        else if (w[t] != w[first]) return false;
    }
    return true;
}

// whether a concat of these tiles (their iso, nvals, vx and tcode fields) into type ccode is iso.
// d_recs: the records on the device when they are already there (matrix path), else nullptr
bool tile_concat_iso(const std::vector<tile_rec> &recs, const tile_rec *d_recs, int ccode) {
    int64_t with = 0;
    for (const tile_rec &r : recs) {
        if (r.nvals <= 0) continue;
        if (!r.iso) return false;
        with++;
    }
    if (with <= 1) return with == 1;
    gb_scratch s;
    const int64_t nt = (int64_t)recs.size();
    if (!d_recs) {
        tile_rec *d = (tile_rec *)s.get<char>(nt * sizeof(tile_rec));
        gb_copy_h2d(d, recs.data(), nt * sizeof(tile_rec));
        d_recs = d;
    }
    unsigned long long *out = s.get<unsigned long long>(nt);
    gb_with_type(ccode, [&](auto z) {
        using D = decltype(z);
        hipLaunchKernelGGL((k_tile_iso_gather<D>), dim3(gb_grid(nt, TILE_BLOCK, 64)), dim3(TILE_BLOCK), 0,
                           gb_stream(), nt, d_recs, out);
    });
    GB_LAUNCH_CHECK();
    std::vector<unsigned long long> w(nt);
    gb_copy_d2h(w.data(), out, nt * sizeof(unsigned long long));
    std::vector<int64_t> nv(nt);
    for (int64_t t = 0; t < nt; t++) nv[t] = recs[t].nvals;
    return tile_values_equal(w, nv);
}

// the shapes of the tiles of a concat, checked against each other and against C
void concat_dims(tile_dims &D, GB_Obj *C, const std::vector<GB_Obj *> &T, int64_t m, int64_t n) {
    std::vector<int64_t> nr(m), nc(n);
    for (int64_t i = 0; i < m; i++) nr[i] = T[i * n]->nrows;
    for (int64_t j = 0; j < n; j++) nc[j] = gb_ncols_of(T[j]);
    for (int64_t i = 0; i < m; i++)
        for (int64_t j = 0; j < n; j++)
            GB_REQUIRE(T[i * n + j]->nrows == nr[i] && gb_ncols_of(T[i * n + j]) == nc[j], GrB_DIMENSION_MISMATCH,
                       "tiles of a tile-row must have the same number of rows, tiles of a tile-column the same "
                       "number of columns");
    D.m = m;
    D.n = n;
    tile_bounds(D.rb, nr, C->nrows, "the tiles' rows do not add up to the output's");
    tile_bounds(D.cb, nc, gb_ncols_of(C), "the tiles' columns do not add up to the output's");
}

void concat_matrix(GB_Obj *C, const std::vector<GB_Obj *> &T, const tile_dims &D) {
    const int64_t m = D.m, n = D.n, nt = m * n;
    const int ccode = C->type->code;
    std::unique_ptr<gb_csr_view[]> views(new gb_csr_view[nt]);
    std::vector<tile_rec> recs(nt);
    std::vector<int64_t> ebase(m + 1, 0), cbase(nt + 1, 0);
    int64_t soff = 0;
    for (int64_t i = 0; i < m; i++) {
        ebase[i + 1] = ebase[i];
        for (int64_t j = 0; j < n; j++) {
            const int64_t t = i * n + j;
            gb_csr_view &v = views[t];
            gb_get_csr(v, T[t]);
            tile_rec &r = recs[t];
            r.rp = v.rowptr;
            r.ci = v.colidx;
            r.vx = v.vals;
            r.nrows = v.nrows;
            r.nvals = v.nvals;
            r.soff = soff;
            r.ebase = ebase[i + 1];
            r.coff = (int32_t)D.cb[j];
            r.tcode = v.tcode;
            r.iso = v.iso;
            r.pad = 0;
            soff += v.nrows;
            ebase[i + 1] += v.nvals;
            cbase[t + 1] = cbase[t] + (v.nvals + TILE_WPI * 64 - 1) / (TILE_WPI * 64);
        }
    }
    const int64_t total = ebase[m], nrows = C->nrows, ncols = gb_ncols_of(C);
    gb_stat_set("concat_bitmap", 0);
    if (total == 0) {
        gb_mat_result E = gb_empty_mat_result(nrows, ncols, ccode);
        gb_stat_set("concat_iso", 0);
        gb_install_csr(C, nrows, ncols, 0, E.rowptr, E.colidx, E.vals, false);
        return;
    }
    gb_scratch s;
    tile_upload up;
    up.add(recs.data(), nt * sizeof(tile_rec));
    up.add(D.rb.data(), (m + 1) * sizeof(int64_t));
    up.add(ebase.data(), (m + 1) * sizeof(int64_t));
    up.add(cbase.data(), (nt + 1) * sizeof(int64_t));
    const int64_t *dev = up.send(s);
    const tile_rec *d_recs = (const tile_rec *)(dev + up.off[0]);
    const bool iso = tile_concat_iso(recs, d_recs, ccode);
    gb_stat_set("concat_iso", iso);
    gb_mat_result R = gb_new_mat_result(nrows, ncols, ccode, total, iso);
    int64_t *start = n == 1 ? nullptr : s.get<int64_t>(soff);
    hipLaunchKernelGGL(k_concat_rowptr, dim3(gb_grid(nrows + 1, TILE_BLOCK, TILE_GRID_CAP)), dim3(TILE_BLOCK), 0,
                       gb_stream(), nrows, total, m, n, d_recs, dev + up.off[1], dev + up.off[2], R.rowptr, start);
    GB_LAUNCH_CHECK();
    const int64_t nchunks = cbase[nt];
    // a wave takes a run of chunks (4 or more, once there are that many)
    const unsigned grid = gb_grid((nchunks + 3) / 4, TILE_BLOCK / 64, TILE_GRID_CAP);
    gb_with_type(ccode, [&](auto z) {
        using Dt = decltype(z);
        auto fill = [&](auto vals, auto panels) {
            hipLaunchKernelGGL((k_concat_fill<Dt, decltype(vals)::value, decltype(panels)::value>), dim3(grid),
                               dim3(TILE_BLOCK), 0, gb_stream(), nchunks, nt, d_recs, dev + up.off[3], start, R.colidx,
                               (Dt *)R.vals);
        };
        if (iso && n == 1) fill(std::false_type{}, std::true_type{});
        else if (iso) fill(std::false_type{}, std::false_type{});
        else if (n == 1) fill(std::true_type{}, std::true_type{});
        else fill(std::true_type{}, std::false_type{});
    });
    GB_LAUNCH_CHECK();
    if (iso) {
        for (const tile_rec &r : recs)
            if (r.nvals > 0) {
                gb_cast_array(R.vals, ccode, r.vx, r.tcode, 1);
                break;
            }
    }
    // the tiles were read by work already enqueued: C may be one of them
    gb_install_csr(C, nrows, ncols, total, R.rowptr, R.colidx, R.vals, iso);
}

// C is a vector (or scalar) object: the tiles with rows and a column are pieces of its bitmap
void concat_bitmap(GB_Obj *C, const std::vector<GB_Obj *> &T, const tile_dims &D) {
    const int64_t nt = D.m * D.n, len = C->nrows;
    const int ccode = C->type->code;
    const size_t cs = C->type->size;
    std::unique_ptr<gb_bitmap_view[]> views(new gb_bitmap_view[nt]);
    std::vector<tile_rec> recs(nt);
    std::vector<int64_t> at(nt, 0);
    bool candidate = true;  // no tile with entries is known not to be iso
    for (int64_t t = 0; t < nt; t++) {
        tile_rec &r = recs[t];
        r = tile_rec{};
        const int64_t i = t / D.n, j = t - i * D.n;
        if (D.rb[i + 1] == D.rb[i] || D.cb[j + 1] == D.cb[j]) continue;  // no positions
        gb_bitmap_view &v = views[t];
        gb_get_bitmap(v, T[t]);
        at[t] = D.rb[i];
        r.vx = v.vals;
        r.nrows = v.n;
        r.tcode = v.tcode;
        r.iso = v.iso;
        r.nvals = -1;  // not asked for yet
        if (!v.iso && candidate) {
            r.nvals = gb_nvals(T[t]);
            if (r.nvals > 0) candidate = false;
        }
    }
    bool iso = false;
    if (candidate) {
        for (int64_t t = 0; t < nt; t++)
            if (recs[t].nrows > 0 && recs[t].nvals < 0) recs[t].nvals = gb_nvals(T[t]);
        iso = tile_concat_iso(recs, nullptr, ccode);
    }
    gb_stat_set("concat_bitmap", 1);
    gb_stat_set("concat_iso", iso);
    gb_vec_result R = gb_new_vec_result(len, ccode, iso);
    gb_memset(R.bits, 0, std::max<int64_t>(gb_words(len), 1) * sizeof(uint64_t));
    bool have_value = false;
    for (int64_t t = 0; t < nt; t++) {
        const tile_rec &r = recs[t];
        if (r.nrows <= 0) continue;
        tile_move_bits(views[t].bits, r.nrows, 0, r.nrows, R.bits, at[t], true);
        if (iso) {
            if (!have_value && r.nvals > 0) {
                gb_cast_array(R.dense, ccode, r.vx, r.tcode, 1);
                have_value = true;
            }
        } else if (r.iso) {
            if (r.nvals == 0) continue;  // nothing there to give a value to
            gb_scratch own;
            void *one = own.get<char>(8);
            gb_cast_array(one, ccode, r.vx, r.tcode, 1);
            gb_with_size(cs, [&](auto w) {
                using W = decltype(w);
                hipLaunchKernelGGL((k_tile_fill<W>), dim3(gb_grid(r.nrows, TILE_BLOCK, TILE_GRID_CAP)),
                                   dim3(TILE_BLOCK), 0, gb_stream(), (W *)R.dense, at[t], r.nrows, (const W *)one);
            });
            GB_LAUNCH_CHECK();
        } else {
            gb_cast_array((char *)R.dense + at[t] * cs, ccode, r.vx, r.tcode, r.nrows);
        }
    }
    if (iso && !have_value) gb_memset(R.dense, 0, cs);
    gb_free(R.d_nvals);  // recounted by the install
    gb_install_bitmap(C, len, R.bits, R.dense, iso, nullptr);
}

// everything a split has allocated so far, given back when it fails
struct split_guard {
    std::vector<void *> ptrs;
    std::vector<GB_Obj *> objs;
    bool armed = true;
    template <class P>
    P *keep(P *p) {
        ptrs.push_back((void *)p);
        return p;
    }
    ~split_guard() {
        if (!armed) return;
        for (void *p : ptrs) gb_free(p);
        for (GB_Obj *o : objs) {
            gb_obj_free_storage(o);
            gb_free(o->d_nvals);
            gb_host_slot_release(o->pub);
            o->magic = GB_FREED;
            delete o;
        }
    }
};

void split_matrix(GrB_Matrix *Tiles, GB_Obj *A, const tile_dims &D) {
    const int64_t m = D.m, n = D.n, nt = m * n;
    gb_csr_view v;
    gb_get_csr(v, A);
    const size_t ts = gb_type_size(v.tcode);
    gb_stat_set("split_bitmap", 0);
    std::vector<int64_t> loff(nt + 1, 0);
    for (int64_t t = 0; t < nt; t++) loff[t + 1] = loff[t] + (D.rb[t / n + 1] - D.rb[t / n]) + 1;
    const int64_t nslots = loff[nt];
    split_guard G;
    std::vector<int64_t *> trp(nt);
    std::vector<int32_t *> tci(nt, nullptr);
    std::vector<void *> tvx(nt, nullptr);
    for (int64_t t = 0; t < nt; t++) trp[t] = G.keep(gb_malloc_n<int64_t>(loff[t + 1] - loff[t]));
    gb_scratch s;
    tile_upload up;
    up.add(D.rb.data(), (m + 1) * sizeof(int64_t));
    up.add(D.cb.data(), (n + 1) * sizeof(int64_t));
    up.add(loff.data(), (nt + 1) * sizeof(int64_t));
    up.add(trp.data(), nt * sizeof(int64_t *));
    const int64_t *dev = up.send(s);
    const int64_t *d_rb = dev + up.off[0], *d_cb = dev + up.off[1], *d_loff = dev + up.off[2];
    int32_t *cnt = s.get<int32_t>(nslots);
    int64_t *cut = s.get<int64_t>(nslots);
    int64_t *S = s.get<int64_t>(nslots + 1);
    int64_t *d_totals = s.get<int64_t>(nt);
    const unsigned sgrid = gb_grid(nslots, TILE_BLOCK, TILE_GRID_CAP);
    hipLaunchKernelGGL(k_split_count, dim3(sgrid), dim3(TILE_BLOCK), 0, gb_stream(), nslots, nt, n, d_rb, d_cb, d_loff,
                       v.rowptr, v.colidx, cnt, cut);
    GB_LAUNCH_CHECK();
    gb_exclusive_scan_i32(cnt, 0, S, nslots);
    hipLaunchKernelGGL(k_split_rowptr, dim3(sgrid), dim3(TILE_BLOCK), 0, gb_stream(), nslots, nt, d_loff, S,
                       (int64_t *const *)(dev + up.off[3]), cut, d_totals);
    GB_LAUNCH_CHECK();
    std::vector<int64_t> totals(nt);
    gb_copy_d2h(totals.data(), d_totals, nt * sizeof(int64_t));
    for (int64_t t = 0; t < nt; t++) {
        tci[t] = G.keep(gb_malloc_n<int32_t>(std::max<int64_t>(totals[t], 1)));
        tvx[t] = G.keep(gb_malloc(std::max<int64_t>(v.iso ? 1 : totals[t], 1) * ts));
    }
    if (v.nvals) {
        tile_upload up2;
        up2.add(tci.data(), nt * sizeof(int32_t *));
        up2.add(tvx.data(), nt * sizeof(void *));
        const int64_t *dev2 = up2.send(s);
        const int64_t nchunks = (v.nvals + TILE_WPI * 64 - 1) / (TILE_WPI * 64);
        const unsigned grid = gb_grid((nchunks + 3) / 4, TILE_BLOCK / 64, TILE_GRID_CAP);
        gb_with_size(ts, [&](auto w) {
            hipLaunchKernelGGL((k_split_fill<(int)sizeof(w)>), dim3(grid), dim3(TILE_BLOCK), 0, gb_stream(), v.nrows,
                               v.nvals, m, n, d_rb, d_cb, d_loff, cut, v.rowptr, v.colidx, v.vals, v.iso,
                               (int32_t *const *)(dev2 + up2.off[0]), (void *const *)(dev2 + up2.off[1]));
        }, true);  // any other size: not implemented
        GB_LAUNCH_CHECK();
    }
    for (int64_t t = 0; t < nt; t++)
        G.objs.push_back(gb_new_object_bare(GB_KIND_MATRIX, A->type, D.rb[t / n + 1] - D.rb[t / n],
                                            D.cb[t % n + 1] - D.cb[t % n]));
    G.armed = false;  // nothing below throws: the tiles take the storage
    for (int64_t t = 0; t < nt; t++) {
        GB_Obj *o = G.objs[t];
        gb_install_csr(o, o->nrows, o->ncols, totals[t], trp[t], tci[t], tvx[t], v.iso);
        Tiles[t] = (GrB_Matrix)o;
    }
}

// A is a vector object: m pieces of its bitmap, each a vector
void split_bitmap(GrB_Matrix *Tiles, GB_Obj *A, const tile_dims &D) {
    GB_REQUIRE(D.n == 1, GrB_DIMENSION_MISMATCH, "a vector is split along its one dimension");
    const int64_t m = D.m;
    const size_t ts = A->type->size;
    gb_stat_set("split_bitmap", 1);
    split_guard G;
    for (int64_t i = 0; i < m; i++) {
        const int64_t at = D.rb[i], len = D.rb[i + 1] - at;
        if (!A->dense) {  // no entry was ever written
            G.objs.push_back(gb_new_object(GB_KIND_VECTOR, A->type, len, 1));
            continue;
        }
        GB_Obj *o = gb_new_object_bare(GB_KIND_VECTOR, A->type, len, 1);
        G.objs.push_back(o);
        o->d_nvals = gb_malloc_n<int64_t>(1);
        uint64_t *bits = G.keep(gb_malloc_n<uint64_t>(std::max<int64_t>(gb_words(len), 1)));
        void *dense = G.keep(gb_malloc(std::max<int64_t>(A->iso ? 1 : len, 1) * ts));
        tile_move_bits(A->bits, A->nrows, at, len, bits, 0, false);
        if (len == 0) gb_memset(bits, 0, sizeof(uint64_t));
        if (A->iso) gb_copy_d2d(dense, A->dense, ts);
        else gb_copy_d2d(dense, (const char *)A->dense + at * ts, len * ts);
        gb_install_bitmap(o, len, bits, dense, A->iso, nullptr);  // allocates nothing: o has its counter
        G.ptrs.clear();                                           // the piece owns them now
    }
    G.armed = false;
    for (int64_t i = 0; i < m; i++) Tiles[i] = (GrB_Matrix)G.objs[i];
}

}  // namespace

extern "C" {

GrB_Info GxB_Matrix_concat(GrB_Matrix C, const GrB_Matrix *Tiles, const GrB_Index m, const GrB_Index n,
                           const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_Obj *Co = gb_obj_check(C);
        GB_REQUIRE(Tiles, GrB_NULL_POINTER, "Tiles is NULL");
        GB_REQUIRE(m > 0 && n > 0, GrB_INVALID_VALUE, "a concat needs at least one tile");
        GB_REQUIRE(m < (1u << 20) && n < (1u << 20) && m * n < (1u << 24), GrB_INVALID_VALUE, "too many tiles");
        gb_read_desc(desc);
        std::vector<GB_Obj *> T(m * n);
        for (size_t t = 0; t < T.size(); t++) T[t] = gb_obj_check(Tiles[t]);
        tile_dims D;
        concat_dims(D, Co, T, (int64_t)m, (int64_t)n);
        if (Co->kind != GB_KIND_MATRIX) concat_bitmap(Co, T, D);
        else concat_matrix(Co, T, D);
    });
}

GrB_Info GxB_Matrix_split(GrB_Matrix *Tiles, const GrB_Index m, const GrB_Index n, const GrB_Index *Tile_nrows,
                          const GrB_Index *Tile_ncols, const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(OBJ(A), [&] {
        GB_Obj *Ao = gb_obj_check(A);
        GB_REQUIRE(Tiles && Tile_nrows && Tile_ncols, GrB_NULL_POINTER, "Tiles, Tile_nrows or Tile_ncols is NULL");
        GB_REQUIRE(m > 0 && n > 0, GrB_INVALID_VALUE, "a split needs at least one tile");
        GB_REQUIRE(m < (1u << 20) && n < (1u << 20) && m * n < (1u << 24), GrB_INVALID_VALUE, "too many tiles");
        gb_read_desc(desc);
        for (GrB_Index t = 0; t < m * n; t++) Tiles[t] = nullptr;
        const int64_t lim = (int64_t)1 << 62;
        std::vector<int64_t> nr(m), nc(n);
        for (GrB_Index i = 0; i < m; i++) nr[i] = Tile_nrows[i] < (GrB_Index)lim ? (int64_t)Tile_nrows[i] : lim;
        for (GrB_Index j = 0; j < n; j++) nc[j] = Tile_ncols[j] < (GrB_Index)lim ? (int64_t)Tile_ncols[j] : lim;
        tile_dims D;
        D.m = (int64_t)m;
        D.n = (int64_t)n;
        tile_bounds(D.rb, nr, Ao->nrows, "Tile_nrows does not add up to the rows of A");
        tile_bounds(D.cb, nc, gb_ncols_of(Ao), "Tile_ncols does not add up to the columns of A");
        if (Ao->kind != GB_KIND_MATRIX) split_bitmap(Tiles, Ao, D);
        else split_matrix(Tiles, Ao, D);
    });
}

}  // extern "C"
