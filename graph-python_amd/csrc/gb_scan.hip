// gb_scan.hip -- GxB_Matrix_scan / GxB_Vector_scan: the inclusive prefix scan of every row
// (column, vector) under a monoid.
//   reference core/ss/matrix.py:3701-3715, core/ss/vector.py:1365-1375, core/ss/prefix_scan.py
//
// C has A's structure; C(i, j) folds row i's stored values at columns <= j, in ascending column
// order, in the monoid's type.  The rows' lengths do not change, so the row pointers and nvals
// are A's: a matrix scan reads nothing back from the device.
//
// Association order.  It is a function of the entry's position p (from 0) among its row's stored
// entries alone, and it is the order of ss.prefix_scan's level schedule, so floats keep their bits.
// Write n = p + 1 in binary.  Every set bit, from the highest down, stands for the next aligned
// block of 2^k entries, folded as a balanced pairwise tree (left half (+) right half); the blocks
// are combined left to right, largest first.  With B(k, n) the tree of the 2^k entries that end at
// position n - 1 and P(n) the result of the first n entries:
//     P(n) = B(k, n)                   if n = 2^k
//     P(n) = P(n - 2^k) (+) B(k, n)    otherwise, k the lowest set bit of n
// That is a Brent-Kung up-sweep (the trees: scan_up) and down-sweep (scan_down: the positions
// whose lowest set bit is k, from the highest k down; their left neighbour P(n - 2^k) is final by
// then).  Both read only to the left, so what a lane past a row's end holds reaches no result,
// and the bits of an output depend on its row's values up to its position and on nothing else.
//
// The order nests.  For n = 64 b + r, 0 < r < 64, the first blocks are those of b -- P(64 b),
// the carry -- and the fold goes on through r's blocks: the down-sweep of a 64-entry block takes
// the carry where its lane r = 2^k would take nothing (it is not "carry (+) local scan", which
// associates differently).  For r = 64 the result is P(64 (b + 1)), which the same scan one level
// up produced, over the blocks' totals: a balanced tree of 2^k totals of 64-entry trees is the
// tree of 2^(k + 6) entries.  scan_segment does this for up to 4096 entries (64 blocks of 64), and
// the same holds once more between chunks and the segments inside them.
//
// Rows by length, decided per wave (no sort or scan of the row ids):
//   k_scan_wave    a wave reads the bounds of 64 consecutive rows.  Rows of one entry are copied.
//                  Rows of 2 .. wave_max (<= 64) entries are scanned in sub-wave groups of 2, 4,
//                  .., 64 lanes, 64 / G rows at a time, up-sweep and down-sweep over __shfl_up.
//                  Longer rows are appended to their class's list, one atomic per workgroup,
//                  sweep and list: the counters are single addresses.
//   k_scan_block   rows up to block_max (<= 4096): a workgroup per listed row, scan_segment
//                  without a carry: every wave sweeps up aligned 64-entry blocks kept in registers,
//                  wave 0 scans the blocks' totals in LDS, every wave sweeps down with its carry.
//   long rows      (the R-MAT hubs, every large vector) are cut into chunks of scan_chunk entries
//                  (a power of two, 64 .. 4096) aligned to the row's start.  k_scan_plan gives every
//                  row its run of work items, one per chunk; k_scan_total folds every full chunk
//                  of a row of more than one chunk to its tree; those totals are a row of the next
//                  level (at the row's work items), scanned by the same three kernels -- at most
//                  four levels for fewer than 2^31 entries at the default chunk --; k_scan_chunk
//                  then scans every chunk as a segment whose carry and last value come from the
//                  level above.  Three streaming passes over a hub row; hubs are few.
// An entry is read once and written once by the wave and block classes: 2 x sizeof(T) bytes, plus
// the row pointer (8 B per row) and the structure copied to C (4 B per entry, 8 B per row).
// Columnwise: the rows of the cached CSC, and the result back to CSR through gb_transpose_csr.
// ANY returns A's values (each is an "any" of its prefix); an iso A under an idempotent monoid
// gives an iso C and no kernel over the entries runs; under the others the one value is read as
// a broadcast.
//
// Vectors: the bitmap's entries are ranked (gb_bitmap_order: word popcounts and a scan) and
// gathered into a contiguous array, which is scanned as the one row of a matrix whose row pointer
// {0, nvals} is written on the device, and scattered to the dense result under u's bitmap.
#include <algorithm>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define SCAN_BLOCK 256
#define SCAN_WAVES (SCAN_BLOCK / 64)
#define SCAN_WAVE_CAP 64
#define SCAN_BLOCK_CAP 4096
#define SCAN_CHUNK_CAP 4096
#define SCAN_BPW (SCAN_BLOCK_CAP / 64 / SCAN_WAVES)  // 64-entry blocks of a segment per wave
#define SCAN_LEVELS 8

namespace {

struct scan_row {
    int64_t start, len;
};

template <class T>
GB_DEV T scan_from_left(T v, int d) {  // the value of lane - d
    if constexpr (sizeof(T) == 8) {
        unsigned long long b;
        __builtin_memcpy(&b, &v, 8);
        b = __shfl_up(b, (unsigned)d);
        __builtin_memcpy(&v, &b, 8);
    } else {
        unsigned b = 0;
        __builtin_memcpy(&b, &v, sizeof(T));
        b = __shfl_up(b, (unsigned)d);
        __builtin_memcpy(&v, &b, sizeof(T));
    }
    return v;
}

// position t (from 0) ends up with B(k, t + 1), k the lowest set bit of t + 1 (at most `levels`)
template <class T>
GB_DEV T scan_up(int mon, T v, int t, int levels) {
    for (int k = 0; k < levels; k++) {
        const T o = scan_from_left(v, 1 << k);
        if (((t + 1) & ((2 << k) - 1)) == 0) v = gb_monoid<T>(mon, o, v);
    }
    return v;
}

// from scan_up's values to P(t + 1); with a carry (what precedes position 0), position 2^k - 1
// folds it in where it has no left neighbour.  Position 2^levels - 1 is left as it is.
template <class T>
GB_DEV T scan_down(int mon, T v, int t, int levels, bool has, T carry) {
    const int r = t + 1;
    for (int k = levels - 1; k >= 0; k--) {
        const T o = scan_from_left(v, 1 << k);
        if ((r & ((2 << k) - 1)) == (1 << k)) {
            if (r > (1 << k)) v = gb_monoid<T>(mon, o, v);
            else if (has) v = gb_monoid<T>(mon, carry, v);
        }
    }
    return v;
}

// A workgroup scans the seglen <= 4096 entries from s.  has: `carry` is the fold of everything
// before s in the row; hasF: the segment is a full chunk, whose last result is F (the level above
// computed it).  Every thread of the workgroup calls this with the same arguments.
template <class T>
GB_DEV void scan_segment(int mon, const T *__restrict__ in, bool iso, T *__restrict__ out, int64_t s, int seglen,
                         bool has, T carry, bool hasF, T F, T *tot, T *pre) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = (seglen + 63) >> 6;
    T u[SCAN_BPW];
#pragma unroll
    for (int j = 0; j < SCAN_BPW; j++) {
        const int b = wave + SCAN_WAVES * j;
        u[j] = T();
        if (b < nb) {
            const int q = b * 64 + lane;
            T v = T();
            if (q < seglen) v = in[iso ? 0 : s + q];
            v = scan_up(mon, v, lane, 6);
            u[j] = v;
            if (lane == 63) tot[b] = v;
        }
    }
    __syncthreads();
    if (wave == 0) {  // the blocks' totals, scanned the same way
        T t = lane < nb ? tot[lane] : T();
        t = scan_up(mon, t, lane, 6);
        t = scan_down(mon, t, lane, 6, has, carry);
        if (hasF && lane == nb - 1) t = F;
        pre[lane] = t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_BPW; j++) {
        const int b = wave + SCAN_WAVES * j;
        if (b < nb) {
            const bool ch = has || b > 0;
            const T cin = b > 0 ? pre[b - 1] : carry;
            T v = scan_down(mon, u[j], lane, 6, ch, cin);
            if (lane == 63 && ch) v = pre[b];
            const int q = b * 64 + lane;
            if (q < seglen) out[s + q] = v;
        }
    }
    __syncthreads();
}

struct scan_args {
    int64_t nrows;
    const int64_t *rowptr;
    const void *in;  // the values as the monoid's type (one value when iso)
    void *out;
    bool iso;
    int mon;
    int wave_max, block_max;
    unsigned long long *stats;  // rows of two or more entries per class: wave, block, long
    int64_t *blist, capB;       // rows of the block class
    scan_row *lrows;            // the long rows
    int64_t capL;
};

template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_wave(scan_args a) {
    const T *__restrict__ in = (const T *)a.in;
    T *__restrict__ out = (T *)a.out;
    // The counters are single addresses: an atomic per wave, sweep and class serialises there.  So
    // the four waves of a workgroup put their list counts of a sweep in LDS and one thread per
    // list takes the slots of all four (buffers alternate with the sweep: a wave that runs ahead
    // writes the other one); the wave class needs no slots and is counted once, at the end.
    __shared__ unsigned cnt[2][2][SCAN_WAVES];
    __shared__ unsigned long long first[2][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    unsigned long long nwave = 0;
    int par = 0;
    for (int64_t bbase = blockIdx.x * (int64_t)SCAN_BLOCK; bbase < a.nrows;
         bbase += (int64_t)gridDim.x * SCAN_BLOCK, par ^= 1) {
        const int64_t base = bbase + wave * 64;
        const int64_t i = base + lane;
        int64_t s = 0, len = 0;
        if (i < a.nrows) {
            s = a.rowptr[i];
            len = a.rowptr[i + 1] - s;
        }
        if (len == 1) out[s] = in[a.iso ? 0 : s];
        const bool isw = len >= 2 && len <= a.wave_max;
        const bool isb = len >= 2 && !isw && len <= a.block_max;
        const bool isl = len >= 2 && !isw && !isb;
        const unsigned long long mw = __ballot(isw), mb = __ballot(isb), ml = __ballot(isl);
        nwave += __popcll(mw);
        if (lane == 0) {
            cnt[par][0][wave] = __popcll(mb);
            cnt[par][1][wave] = __popcll(ml);
        }
        __syncthreads();
        if (threadIdx.x < 2) {  // thread 0: the block class's list, thread 1: the long rows'
            unsigned total = 0;
            for (int w = 0; w < SCAN_WAVES; w++) total += cnt[par][threadIdx.x][w];
            if (total) first[par][threadIdx.x] = atomicAdd(&a.stats[1 + threadIdx.x], (unsigned long long)total);
        }
        __syncthreads();
        if (mb) {
            int64_t slot = (int64_t)first[par][0] + __popcll(mb & below);
            for (int w = 0; w < wave; w++) slot += cnt[par][0][w];
            if (isb && slot < a.capB) a.blist[slot] = i;
        }
        if (ml) {
            int64_t slot = (int64_t)first[par][1] + __popcll(ml & below);
            for (int w = 0; w < wave; w++) slot += cnt[par][1][w];
            if (isl && slot < a.capL) a.lrows[slot] = {s, len};
        }
        if (!mw) continue;
        const int ilen = isw ? (int)len : 0;
        for (int lg = 1; lg <= 6; lg++) {
            const int G = 1 << lg;
            unsigned long long m = __ballot(ilen > (G >> 1) && ilen <= G);
            const int g = lane >> lg, t = lane & (G - 1);
            while (m) {  // 64 / G rows at a time: group g takes the g-th set bit
                unsigned long long rest = m;
                int src = -1;
                for (int n = 0; n < (64 >> lg) && rest; n++) {
                    const int bit = __ffsll((long long)rest) - 1;
                    if (n == g) src = bit;
                    rest &= rest - 1;
                }
                m = rest;
                const int from = src < 0 ? 0 : src;
                const int64_t rs = (int64_t)__shfl((unsigned long long)s, from);
                int rl = __shfl(ilen, from);
                if (src < 0) rl = 0;
                T v = T();
                if (t < rl) v = in[a.iso ? 0 : rs + t];
                v = scan_up(a.mon, v, t, lg);
                v = scan_down(a.mon, v, t, lg, false, T());
                if (t < rl) out[rs + t] = v;
            }
        }
    }
    if (lane == 0 && nwave) atomicAdd(&a.stats[0], nwave);
}

template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_block(scan_args a) {
    __shared__ T tot[64], pre[64];
    const int64_t cnt = min((int64_t)a.stats[1], a.capB);
    for (int64_t b = blockIdx.x; b < cnt; b += gridDim.x) {
        const int64_t i = a.blist[b];
        const int64_t s = a.rowptr[i];
        const int len = (int)min(a.rowptr[i + 1] - s, (int64_t)SCAN_BLOCK_CAP);
        scan_segment<T>(a.mon, (const T *)a.in, a.iso, (T *)a.out, s, len, false, T(), false, T(), tot, pre);
    }
}

// One level of the long rows.  Its rows lie in `in` / `out` (the values at level 0, the totals of
// the level below and their scan after that); row r has the work items base[r] .. base[r] +
// ceil(len / chunk) - 1, and desc maps a work item back to its row.  A row of more than one chunk
// is a row of the level above: there it starts at base[r] (so the total of chunk c lies at the
// chunk's own work item) and has floor(len / chunk) entries.
struct scan_level {
    const scan_row *rows;
    const unsigned long long *nrows_d;
    int64_t cap_rows;
    int64_t *base, *desc;
    unsigned long long *nwork_d;
    int64_t cap_work;
    const void *in;
    void *out;
    bool iso;
    int mon, chunk;
    scan_row *up_rows;  // the level above (nullptr: no row here can have more than one chunk)
    unsigned long long *up_nrows_d;
    int64_t up_cap_rows;
    void *up_tot;
    const void *up_pre;
};

__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_plan(scan_level L) {
    __shared__ int64_t sbase;
    const int64_t cnt = min((int64_t)*L.nrows_d, L.cap_rows);
    for (int64_t r = blockIdx.x; r < cnt; r += gridDim.x) {
        const int64_t len = L.rows[r].len;
        const int64_t nchunk = (len + L.chunk - 1) / L.chunk;
        if (threadIdx.x == 0) {
            sbase = (int64_t)atomicAdd(L.nwork_d, (unsigned long long)nchunk);
            L.base[r] = sbase;
            if (len > L.chunk && L.up_rows) {
                const int64_t slot = (int64_t)atomicAdd(L.up_nrows_d, 1ull);
                if (slot < L.up_cap_rows) L.up_rows[slot] = {sbase, len / L.chunk};
            }
        }
        __syncthreads();
        for (int64_t c = threadIdx.x; c < nchunk; c += SCAN_BLOCK)
            if (sbase + c < L.cap_work) L.desc[sbase + c] = r;
        __syncthreads();
    }
}

// the tree of every full chunk of the rows of more than one chunk, to the level above
template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_total(scan_level L) {
    __shared__ T tot[64];
    const T *__restrict__ in = (const T *)L.in;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = L.chunk >> 6;
    const int64_t cnt = min((int64_t)*L.nwork_d, L.cap_work);
    for (int64_t w = blockIdx.x; w < cnt; w += gridDim.x) {
        const int64_t r = L.desc[w], c = w - L.base[r];
        const scan_row row = L.rows[r];
        if (row.len <= L.chunk || (c + 1) * L.chunk > row.len) continue;
        const int64_t s = row.start + c * L.chunk;
        for (int b = wave; b < nb; b += SCAN_WAVES) {
            T v = in[L.iso ? 0 : s + b * 64 + lane];
            v = scan_up(L.mon, v, lane, 6);
            if (lane == 63) tot[b] = v;
        }
        __syncthreads();
        if (wave == 0) {
            T t = lane < nb ? tot[lane] : T();
            t = scan_up(L.mon, t, lane, 6);
            if (lane == nb - 1) ((T *)L.up_tot)[w] = t;
        }
        __syncthreads();
    }
}

template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_chunk(scan_level L) {
    __shared__ T tot[64], pre[64];
    const T *__restrict__ up = (const T *)L.up_pre;
    const int64_t cnt = min((int64_t)*L.nwork_d, L.cap_work);
    for (int64_t w = blockIdx.x; w < cnt; w += gridDim.x) {
        const int64_t r = L.desc[w], c = w - L.base[r];
        const scan_row row = L.rows[r];
        const int64_t done = c * L.chunk;
        if (done >= row.len) continue;  // cannot be: the row has ceil(len / chunk) work items
        const int seglen = (int)min((int64_t)L.chunk, row.len - done);
        const bool above = row.len > L.chunk && up;
        const bool has = above && c > 0, hasF = above && seglen == L.chunk;
        const T carry = has ? up[w - 1] : T();
        const T F = hasF ? up[w] : T();
        scan_segment<T>(L.mon, (const T *)L.in, L.iso, (T *)L.out, row.start + done, seglen, has, carry, hasF, F, tot,
                        pre);
    }
}

// rows per class of the last call, on the device: read only when a counter is asked for
unsigned long long *g_scan_stats = nullptr;

int scan_knob(const char *key, int dflt) {
    const int64_t k = gb_knob(key);
    return k > 0 && k < dflt ? (int)k : dflt;
}

int scan_chunk_knob() {  // a power of two, 64 .. 4096
    const int k = scan_knob("scan_chunk", SCAN_CHUNK_CAP);
    int c = 64;
    while (c * 2 <= k) c *= 2;
    return c;
}

void scan_reset_stats() {
    if (!g_scan_stats) g_scan_stats = gb_malloc_n<unsigned long long>(3);
    gb_memset(g_scan_stats, 0, 3 * sizeof(unsigned long long));
}

// out = the scan of every row of the CSR rows `rowptr` over `in`; at most nvcap entries (the
// host's bound: the lists and the levels are sized by it, the kernels read the device's counts)
template <class T>
void scan_rows(int64_t nrows, int64_t nvcap, const int64_t *rowptr, const T *in, bool iso, T *out, int mon) {
    gb_scratch s;
    scan_args a{};
    a.nrows = nrows;
    a.rowptr = rowptr;
    a.in = in;
    a.out = out;
    a.iso = iso;
    a.mon = mon;
    a.wave_max = scan_knob("scan_wave_max", SCAN_WAVE_CAP);
    a.block_max = std::max(a.wave_max, scan_knob("scan_block_max", SCAN_BLOCK_CAP));
    a.stats = g_scan_stats;
    // a row of a class is longer than the class below allows: that bounds the lists
    a.capB = std::min(nrows, nvcap / (a.wave_max + 1));
    a.capL = std::min(nrows, nvcap / (a.block_max + 1));
    a.blist = s.get<int64_t>(a.capB);
    a.lrows = s.get<scan_row>(a.capL);
    hipLaunchKernelGGL(k_scan_wave<T>, dim3(gb_sort_grid(nrows, SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, gb_stream(), a);
    GB_LAUNCH_CHECK();
    if (a.capB) {
        hipLaunchKernelGGL(k_scan_block<T>, dim3(gb_sort_grid(a.capB, 1)), dim3(SCAN_BLOCK), 0, gb_stream(), a);
        GB_LAUNCH_CHECK();
    }
    if (!a.capL) return;

    const int chunk = scan_chunk_knob();
    scan_level lv[SCAN_LEVELS];
    gb_scratch ls[SCAN_LEVELS];
    unsigned long long *counts = s.get<unsigned long long>(2 * SCAN_LEVELS);  // per level: work items, rows above
    gb_memset(counts, 0, 2 * SCAN_LEVELS * sizeof(unsigned long long));
    int nlev = 0;
    int64_t entries = nvcap, cap_rows = a.capL;
    const scan_row *rows = a.lrows;
    const unsigned long long *nrows_d = a.stats + 2;
    const void *lin = in;
    void *lout = out;
    bool liso = iso;
    while (true) {
        scan_level &L = lv[nlev];
        L = scan_level{};
        L.rows = rows;
        L.nrows_d = nrows_d;
        L.cap_rows = cap_rows;
        L.cap_work = entries / chunk + cap_rows;
        L.base = ls[nlev].get<int64_t>(cap_rows);
        L.desc = ls[nlev].get<int64_t>(L.cap_work);
        L.nwork_d = counts + 2 * nlev;
        L.in = lin;
        L.out = lout;
        L.iso = liso;
        L.mon = mon;
        L.chunk = chunk;
        // a row of the level above has more than chunk entries here
        const int64_t up_rows = std::min(cap_rows, entries / ((int64_t)chunk + 1));
        nlev++;
        if (up_rows < 1) break;
        GB_REQUIRE(nlev < SCAN_LEVELS, GrB_NOT_IMPLEMENTED, "scan: too many levels of chunks");
        L.up_rows = ls[nlev - 1].get<scan_row>(up_rows);
        L.up_nrows_d = counts + 2 * (nlev - 1) + 1;
        L.up_cap_rows = up_rows;
        T *up_tot = ls[nlev - 1].get<T>(L.cap_work), *up_pre = ls[nlev - 1].get<T>(L.cap_work);
        L.up_tot = up_tot;
        L.up_pre = up_pre;
        rows = L.up_rows;
        nrows_d = L.up_nrows_d;
        cap_rows = up_rows;
        entries /= chunk;
        lin = up_tot;
        lout = up_pre;
        liso = false;
    }
    for (int l = 0; l < nlev; l++) {
        hipLaunchKernelGGL(k_scan_plan, dim3(gb_sort_grid(lv[l].cap_rows, 1)), dim3(SCAN_BLOCK), 0, gb_stream(), lv[l]);
        if (lv[l].up_rows)
            hipLaunchKernelGGL(k_scan_total<T>, dim3(gb_sort_grid(lv[l].cap_work, 1)), dim3(SCAN_BLOCK), 0, gb_stream(),
                               lv[l]);
        GB_LAUNCH_CHECK();
    }
    for (int l = nlev - 1; l >= 0; l--) {
        hipLaunchKernelGGL(k_scan_chunk<T>, dim3(gb_sort_grid(lv[l].cap_work, 1)), dim3(SCAN_BLOCK), 0, gb_stream(),
                           lv[l]);
        GB_LAUNCH_CHECK();
    }
}

bool scan_idempotent(int mon) {
    switch (mon) {
    case GBAMD_MON_MIN:
    case GBAMD_MON_MAX:
    case GBAMD_MON_ANY:
    case GBAMD_MON_LOR:
    case GBAMD_MON_LAND:
    case GBAMD_MON_BOR:
    case GBAMD_MON_BAND: return true;
    default: return false;
    }
}

void scan_check_monoid(GrB_Monoid op) {
    GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid monoid");
}

void matrix_scan(GB_Obj *C, GrB_Monoid op, GB_Obj *A, const gb_desc &d) {
    scan_check_monoid(op);
    GB_REQUIRE(A->kind == GB_KIND_MATRIX && C->kind == GB_KIND_MATRIX, GrB_INVALID_OBJECT, "not a matrix");
    GB_REQUIRE(C->nrows == A->nrows && C->ncols == A->ncols, GrB_DIMENSION_MISMATCH,
               "output dimensions do not match A");
    const int mon = op->mcode, tcode = op->type->code;
    gb_csr_view v;
    if (d.tran0) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    const int64_t nr = v.nrows, nv = v.nvals;
    const size_t ts = gb_type_size(tcode);
    scan_reset_stats();
    const gb_desc d0;
    if (nv == 0) {
        gb_mat_result E = gb_empty_mat_result(C->nrows, C->ncols, tcode);
        gb_writeback_matrix(C, E, nullptr, d0, nullptr);
        return;
    }
    const bool oiso = v.iso && scan_idempotent(mon);
    void *vals = gb_malloc((oiso ? 1 : nv) * ts);
    {
        gb_scratch s;
        const void *xin = gb_view_vals_as(v, tcode, s);
        if (oiso) {
            gb_copy_d2d(vals, xin, ts);
        } else if (mon == GBAMD_MON_ANY) {  // every entry is an "any" of its prefix
            gb_copy_d2d(vals, xin, nv * ts);
        } else {
            gb_with_type(tcode, [&](auto z) {
                using T = decltype(z);
                scan_rows<T>(nr, nv, v.rowptr, (const T *)xin, v.iso, (T *)vals, mon);
            });
        }
    }
    gb_mat_result T;
    T.nrows = C->nrows;
    T.ncols = C->ncols;
    T.nvals = nv;
    T.tcode = tcode;
    T.iso = oiso;
    if (d.tran0) {  // the scanned rows are A's columns: back to CSR
        gb_transpose_csr(v.nrows, v.ncols, nv, v.rowptr, v.colidx, vals, ts, oiso, &T.rowptr, &T.colidx, &T.vals);
        gb_free(vals);
    } else {
        T.rowptr = gb_malloc_n<int64_t>(nr + 1);
        gb_copy_d2d(T.rowptr, v.rowptr, (nr + 1) * sizeof(int64_t));
        T.colidx = gb_malloc_n<int32_t>(nv);
        gb_copy_d2d(T.colidx, v.colidx, nv * sizeof(int32_t));
        T.vals = vals;
    }
    gb_writeback_matrix(C, T, nullptr, d0, nullptr);
}

// ------------------------------------------------------------------ vectors
// the entries in index order, contiguous, and the one row they form
template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_vec_gather(int64_t n, const int64_t *__restrict__ off,
                                                                const int64_t *__restrict__ idx,
                                                                const T *__restrict__ x, bool iso,
                                                                T *__restrict__ packed, int64_t *__restrict__ rowptr) {
    const int64_t nvals = off[(n + 63) >> 6];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rowptr[0] = 0;
        rowptr[1] = nvals;
    }
    for (int64_t k = blockIdx.x * (int64_t)SCAN_BLOCK + threadIdx.x; k < nvals; k += (int64_t)gridDim.x * SCAN_BLOCK)
        packed[k] = x[iso ? 0 : idx[k]];
}

// the dense result (zeroed by the caller) under u's bitmap, and the count
template <class T>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_vec_scatter(int64_t n, const int64_t *__restrict__ off,
                                                                 const int64_t *__restrict__ idx,
                                                                 const T *__restrict__ packed, T *__restrict__ dense,
                                                                 const uint64_t *__restrict__ ubits,
                                                                 uint64_t *__restrict__ wbits, int64_t *wcount) {
    const int64_t nvals = off[(n + 63) >> 6], nw = (n + 63) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) *wcount = nvals;
    for (int64_t k = blockIdx.x * (int64_t)SCAN_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * SCAN_BLOCK) {
        if (packed && k < nvals) dense[idx[k]] = packed[k];
        if (k < nw) {
            uint64_t b = ubits[k];
            if (k == nw - 1 && (n & 63)) b &= (1ull << (n & 63)) - 1;
            wbits[k] = b;
        }
    }
}

void vector_scan(GB_Obj *W, GrB_Monoid op, GB_Obj *U) {
    scan_check_monoid(op);
    GB_REQUIRE(gb_ncols_of(U) == 1 && gb_ncols_of(W) == 1, GrB_DIMENSION_MISMATCH, "not a vector");
    GB_REQUIRE(W->nrows == U->nrows, GrB_DIMENSION_MISMATCH, "output size does not match u");
    const int mon = op->mcode, tcode = op->type->code;
    gb_bitmap_view uv;
    gb_get_bitmap(uv, U);
    const int64_t n = uv.n;
    const size_t ts = gb_type_size(tcode);
    scan_reset_stats();
    const bool wiso = uv.iso && scan_idempotent(mon);
    gb_vec_result T = gb_new_vec_result(n, tcode, wiso);
    if (n == 0) {
        gb_memset(T.d_nvals, 0, sizeof(int64_t));
    } else {
        gb_scratch s;
        const void *xin = gb_bitmap_vals_as(uv, tcode, s);
        int64_t *idx, *off;
        gb_bitmap_order(n, uv.bits, nullptr, 0, false, 0, 0, s, &idx, &off);
        const unsigned grid = gb_sort_grid(n, SCAN_BLOCK);
        gb_with_type(tcode, [&](auto z) {
            using X = decltype(z);
            const X *packed = nullptr;
            if (wiso) {
                gb_copy_d2d(T.dense, xin, ts);
            } else if (mon == GBAMD_MON_ANY) {  // u's own values, cast
                gb_copy_d2d(T.dense, xin, n * ts);
            } else {
                X *pk = s.get<X>(n), *res = s.get<X>(n);
                int64_t *rowptr = s.get<int64_t>(2);
                hipLaunchKernelGGL(k_scan_vec_gather<X>, dim3(grid), dim3(SCAN_BLOCK), 0, gb_stream(), n,
                                   (const int64_t *)off, (const int64_t *)idx, (const X *)xin, uv.iso, pk, rowptr);
                GB_LAUNCH_CHECK();
                scan_rows<X>(1, n, rowptr, pk, false, res, mon);
                gb_memset(T.dense, 0, n * ts);
                packed = res;
            }
            hipLaunchKernelGGL(k_scan_vec_scatter<X>, dim3(grid), dim3(SCAN_BLOCK), 0, gb_stream(), n,
                               (const int64_t *)off, (const int64_t *)idx, packed, (X *)T.dense, uv.bits, T.bits,
                               T.d_nvals);
            GB_LAUNCH_CHECK();
        });
    }
    const gb_desc d0;
    gb_writeback_vector(W, T, nullptr, d0, nullptr, false);
}

}  // namespace

bool gb_scan_stat(const char *key, int64_t *value) {
    static const char *names[3] = {"stat_scan_rows_wave", "stat_scan_rows_block", "stat_scan_rows_long"};
    for (int k = 0; k < 3; k++) {
        if (strcmp(key, names[k])) continue;
        *value = g_scan_stats ? gb_read_i64((const int64_t *)g_scan_stats + k) : 0;
        return true;
    }
    // the class bounds and the chunk read back as their defaults while unset
    if (!strcmp(key, "scan_wave_max")) {
        *value = scan_knob(key, SCAN_WAVE_CAP);
        return true;
    }
    if (!strcmp(key, "scan_block_max")) {
        *value = std::max(scan_knob("scan_wave_max", SCAN_WAVE_CAP), scan_knob(key, SCAN_BLOCK_CAP));
        return true;
    }
    if (!strcmp(key, "scan_chunk")) {
        *value = scan_chunk_knob();
        return true;
    }
    return false;
}

extern "C" {

GrB_Info GxB_Matrix_scan(GrB_Matrix C, const GrB_Monoid op, const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(OBJ(C), [&] {
        GB_REQUIRE(C && op && A, GrB_NULL_POINTER, "C, op or A is NULL");
        matrix_scan(gb_obj_check(C), op, gb_obj_check(A), gb_read_desc(desc));
    });
}

GrB_Info GxB_Vector_scan(GrB_Vector w, const GrB_Monoid op, const GrB_Vector u, const GrB_Descriptor desc) {
    return gb_api(OBJ(w), [&] {
        GB_REQUIRE(w && op && u, GrB_NULL_POINTER, "w, op or u is NULL");
        gb_read_desc(desc);
        vector_scan(gb_obj_check(w), op, gb_obj_check(u));
    });
}

}  // extern "C"
