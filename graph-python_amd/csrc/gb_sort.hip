// gb_sort.hip -- GxB_Matrix_sort / GxB_Vector_sort: every row (column, vector) ordered by value.
//   reference core/ss/matrix.py:3991-4055, core/ss/vector.py:1562
//
// C(i, r) = the value of rank r in row i, P(i, r) = the column it came from; rows keep their
// lengths, so the row pointers are A's and nvals is known on the host: a matrix sort reads
// nothing back from the device.
//
// Keys.  A value of the operator's type becomes an unsigned key of the same width whose integer
// order is the value order (sign bit flipped for signed integers, the usual transform for
// floats with -0.0 made +0.0 for the key only); GrB_GT complements it, so every path sorts
// ascending.  Equal values keep ascending original index.  CSR rows are in ascending column
// order (import checks it, every producer keeps it), so "original index" is the position in the
// row, and (key, position) is a total order: every path below produces identical bits.
//
// Rows by length, decided per wave (no sort or scan of the row ids):
//   k_sort_wave    a wave reads the bounds of 64 consecutive rows.  Rows of one entry are copied.
//                  Rows of 2 .. wave_max (<= 64) entries are sorted in sub-wave groups of 2, 4,
//                  .., 64 lanes, 64 / G rows at a time, by a register bitonic network over
//                  cross-lane exchanges.  Bitonic sort is not stable: it compares (key, position),
//                  one 64-bit word for types of at most 32 bits, two words for 64-bit types.  Lanes
//                  past the row's end hold a pad above every real element.  Longer rows are
//                  appended (one atomic per wave and class) to the list of their class.
//   k_sort_block   rows up to block_max (<= 2048): a workgroup per listed row, bitonic in LDS.
//                  Rows up to 512 entries get a workgroup of one wave (4 KiB of LDS for the (key,
//                  position) pairs, 6 KiB for 64-bit types: LDS allows 26 such waves per CU and the
//                  barriers cost nothing); longer ones 256 threads and 16 KiB / 24 KiB, 6
//                  workgroups (24 waves) in the 160 KiB of a CU.
//   hipCUB         longer rows (the R-MAT hubs): DeviceSegmentedRadixSort over those rows only,
//                  keys with the entry positions as payload; it is stable.  The segment list has
//                  a host-known capacity (nvals / (block_max + 1)); unused slots are empty.
// Every class writes its outputs itself: C's values gathered from the sorted positions, P's as
// colidx[position], the new column index = the rank.  What was not asked for is not written.
// sort_method = 1 sends every row of two or more entries through hipCUB (the A/B baseline).
// Columnwise: the rows of the cached CSC are sorted and the result returns to CSR through
// gb_transpose_csr.  An iso A has nothing to sort: C is iso, P holds the columns.
//
// Vectors: bitmap compaction (word popcounts, scan), key build, gb_sort_pairs_u64 over all n
// slots (the unused ones padded with the largest key, which a stable sort leaves at the end),
// and a dense scatter that also writes the prefix-of-ones bitmap and the device count.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

#define SORT_BLOCK 256
#define SORT_WAVE_CAP 64
#define SORT_BLOCK_CAP 2048
#define SORT_SMALL_CAP 512  // rows up to here take one wave of their own in the workgroup class

namespace {

template <class X>
GB_DEV uint64_t sort_key(X x) {
    if constexpr (std::is_same<X, bool>::value) {
        return x ? 1 : 0;
    } else if constexpr (std::is_same<X, float>::value) {
        uint32_t b = __float_as_uint(x);
        if ((b << 1) == 0) b = 0;  // -0.0 sorts as +0.0
        return (b & 0x80000000u) ? (uint32_t)~b : (b | 0x80000000u);
    } else if constexpr (std::is_same<X, double>::value) {
        uint64_t b = (uint64_t)__double_as_longlong(x);
        if ((b << 1) == 0) b = 0;
        return (b >> 63) ? ~b : (b | (1ull << 63));
    } else if constexpr (std::is_signed<X>::value) {
        using U = typename std::make_unsigned<X>::type;
        return (U)((U)x ^ (U)((U)1 << (8 * sizeof(X) - 1)));
    } else {
        return (uint64_t)x;
    }
}

// an element of the comparison sorts: (key, position in the row)
template <bool WIDE>
struct sort_elem;
template <>
struct sort_elem<false> {
    uint64_t k;  // key << 32 | position
    GB_DEV static sort_elem make(uint64_t key, uint32_t pos) { return {(key << 32) | pos}; }
    GB_DEV static sort_elem pad(uint32_t pos) { return {(0xffffffffull << 32) | pos}; }
    GB_DEV uint32_t pos() const { return (uint32_t)k; }
    GB_DEV bool less(const sort_elem &o) const { return k < o.k; }
    GB_DEV sort_elem xchg(int j) const { return {(uint64_t)__shfl_xor((unsigned long long)k, j)}; }
};
template <>
struct sort_elem<true> {
    uint64_t k;
    uint32_t p;
    GB_DEV static sort_elem make(uint64_t key, uint32_t pos) { return {key, pos}; }
    GB_DEV static sort_elem pad(uint32_t pos) { return {~0ull, pos}; }
    GB_DEV uint32_t pos() const { return p; }
    GB_DEV bool less(const sort_elem &o) const { return k < o.k || (k == o.k && p < o.p); }
    GB_DEV sort_elem xchg(int j) const {
        return {(uint64_t)__shfl_xor((unsigned long long)k, j), (uint32_t)__shfl_xor((int)p, j)};
    }
};

struct sort_args {
    int64_t nrows, nvals;
    const int64_t *rowptr;
    const int32_t *colidx;
    const void *xin;    // values as the operator's type (keys)
    const void *avals;  // A's own values (moved)
    int vs;             // bytes of one of them
    uint64_t flip;      // xor of the key: all ones of its width for GT
    void *oC;           // sorted values (nullptr: not requested)
    int64_t *oP;        // their columns (nullptr: not requested)
    int32_t *ocol;      // the ranks
    int wave_max, block_max;
    bool all_long;      // sort_method = 1: count only, hipCUB takes every row
    unsigned long long *stats;  // rows per class: wave, block (one wave), long, block (256 threads)
    int64_t *blist, capB;       // rows of the block class up to SORT_SMALL_CAP entries
    int64_t *blist2, capB2;     // its longer rows
    int64_t *lbeg, *lend, capL;  // entry ranges of the long rows
    int64_t *lrow;               // and the rows themselves
    // the trimmed emit of gb_rank_rows (gb_internal.h, gb_rank_job); a sort emits every rank in place:
    // orp = nullptr (the output rows are the input's), m = INT64_MAX, the rest unset
    const int64_t *orp;
    int64_t m;
    bool far, reverse;
    uint8_t *keep;
    uint64_t seed;  // of the random order (X = sort_rnd)
};

// the key type of the random order: nothing is read, the key is a hash of (seed, row, position)
struct sort_rnd {
    uint64_t x;
};

// the key of entry t of the row `row` that starts at s
template <class X>
GB_DEV uint64_t sort_key_at(const sort_args &a, const X *__restrict__ xin, int64_t row, int64_t s, int64_t t) {
    if constexpr (std::is_same<X, sort_rnd>::value) return gb_hash3(a.seed, (uint64_t)row, (uint64_t)t);
    else return sort_key<X>(xin[s + t]) ^ a.flip;
}

// rank t of a row of len entries (its output row starts at os) is input entry p: entry
// u = far ? len-1-t : t of the requested order, emitted when u < m at slot u, or
// min(m, len)-1-u under reverse; with keep it is only marked
GB_DEV void sort_emit(const sort_args &a, int64_t os, int64_t len, int64_t p, int32_t t) {
    const int64_t u = a.far ? len - 1 - t : t;
    if (u >= a.m) return;
    if (a.keep) {
        a.keep[p] = 1;
        return;
    }
    const int64_t slot = a.reverse ? min(a.m, len) - 1 - u : u;
    const int64_t q = os + slot;
    a.ocol[q] = (int32_t)slot;
    if (a.oP) a.oP[q] = a.colidx[p];
    if (a.oC) {
        switch (a.vs) {
        case 1: ((uint8_t *)a.oC)[q] = ((const uint8_t *)a.avals)[p]; break;
        case 2: ((uint16_t *)a.oC)[q] = ((const uint16_t *)a.avals)[p]; break;
        case 4: ((uint32_t *)a.oC)[q] = ((const uint32_t *)a.avals)[p]; break;
        default: ((uint64_t *)a.oC)[q] = ((const uint64_t *)a.avals)[p]; break;
        }
    }
}

// the position of the n-th (from 0) set bit of m; n below popcount(m)
GB_DEV int sort_nth_set(unsigned long long m, int n) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w; w >>= 1) {
        const int c = __popcll(m & (((1ull << w) - 1) << pos));
        if (n >= c) {
            n -= c;
            pos += w;
        }
    }
    return pos;
}

template <class X>
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_wave(sort_args a) {
    constexpr bool WIDE = sizeof(X) == 8;
    using E = sort_elem<WIDE>;
    const X *__restrict__ xin = (const X *)a.xin;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t nwaves = ((int64_t)gridDim.x * SORT_BLOCK) >> 6;
    for (int64_t base = ((blockIdx.x * (int64_t)SORT_BLOCK + threadIdx.x) >> 6) << 6; base < a.nrows;
         base += nwaves << 6) {
        const int64_t i = base + lane;
        int64_t s = 0, len = 0, os = 0;
        if (i < a.nrows) {
            s = a.rowptr[i];
            len = a.rowptr[i + 1] - s;
            os = a.orp ? a.orp[i] : s;
            if (a.keep && len <= a.m) len = 0;  // kept whole by the caller
        }
        if (len == 1 && !a.all_long) sort_emit(a, os, 1, s, 0);
        const bool isl = len >= 2 && (a.all_long || len > a.block_max);
        const bool isw = len >= 2 && !isl && len <= a.wave_max;
        const bool isb = len >= 2 && !isl && !isw && len <= SORT_SMALL_CAP;
        const bool isb2 = len >= 2 && !isl && !isw && !isb;
        const unsigned long long mw = __ballot(isw), mb = __ballot(isb), ml = __ballot(isl), mb2 = __ballot(isb2);
        if (mw && lane == 0) atomicAdd(&a.stats[0], (unsigned long long)__popcll(mw));
        if (mb) {
            unsigned long long b0 = 0;
            if (lane == 0) b0 = atomicAdd(&a.stats[1], (unsigned long long)__popcll(mb));
            b0 = __shfl(b0, 0);
            const int64_t slot = (int64_t)b0 + __popcll(mb & below);
            if (isb && slot < a.capB) a.blist[slot] = i;
        }
        if (mb2) {
            unsigned long long b0 = 0;
            if (lane == 0) b0 = atomicAdd(&a.stats[3], (unsigned long long)__popcll(mb2));
            b0 = __shfl(b0, 0);
            const int64_t slot = (int64_t)b0 + __popcll(mb2 & below);
            if (isb2 && slot < a.capB2) a.blist2[slot] = i;
        }
        if (ml) {
            unsigned long long l0 = 0;
            if (lane == 0) l0 = atomicAdd(&a.stats[2], (unsigned long long)__popcll(ml));
            l0 = __shfl(l0, 0);
            const int64_t slot = (int64_t)l0 + __popcll(ml & below);
            if (isl && !a.all_long && slot < a.capL) {
                a.lbeg[slot] = s;
                a.lend[slot] = s + len;
                a.lrow[slot] = i;
            }
        }
        if (!mw) continue;
        const int ilen = isw ? (int)len : 0;
        for (int lg = 1; lg <= 6; lg++) {
            const int G = 1 << lg;
            const unsigned long long m = __ballot(ilen > (G >> 1) && ilen <= G);
            const int total = __popcll(m);
            const int g = lane >> lg, t = lane & (G - 1);
            for (int done = 0; done < total; done += 64 >> lg) {
                const int n = done + g;
                const int src = n < total ? sort_nth_set(m, n) : 0;
                const int64_t rs = (int64_t)__shfl((unsigned long long)s, src);
                const int64_t ros = (int64_t)__shfl((unsigned long long)os, src);
                int rl = __shfl(ilen, src);
                if (n >= total) rl = 0;
                E e = E::pad((uint32_t)t);
                if (t < rl) e = E::make(sort_key_at<X>(a, xin, base + src, rs, t), (uint32_t)t);
                for (int k = 2; k <= G; k <<= 1) {
                    for (int j = k >> 1; j > 0; j >>= 1) {
                        const E o = e.xchg(j);
                        const bool take_min = ((t & j) == 0) == ((t & k) == 0);
                        if (take_min ? o.less(e) : e.less(o)) e = o;
                    }
                }
                if (t < rl) sort_emit(a, ros, rl, rs + e.pos(), t);
            }
        }
    }
}

// THREADS threads sort one listed row of at most CAP entries at a time
template <class X, int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void k_sort_block(sort_args a) {
    constexpr bool WIDE = sizeof(X) == 8;
    constexpr bool SMALL = CAP == SORT_SMALL_CAP;
    using E = sort_elem<WIDE>;
    __shared__ uint64_t sk[CAP];
    __shared__ uint32_t sp[WIDE ? CAP : 1];
    const X *__restrict__ xin = (const X *)a.xin;
    const int tid = threadIdx.x;
    const int64_t *__restrict__ list = SMALL ? a.blist : a.blist2;
    const int64_t cnt = SMALL ? min((int64_t)a.stats[1], a.capB) : min((int64_t)a.stats[3], a.capB2);
    auto load = [&](int t) {
        E e;
        e.k = sk[t];
        if constexpr (WIDE) e.p = sp[t];
        return e;
    };
    auto store = [&](int t, const E &e) {
        sk[t] = e.k;
        if constexpr (WIDE) sp[t] = e.p;
    };
    for (int64_t b = blockIdx.x; b < cnt; b += gridDim.x) {
        const int64_t i = list[b];
        const int64_t s = a.rowptr[i];
        const int len = (int)min(a.rowptr[i + 1] - s, (int64_t)CAP);
        const int64_t os = a.orp ? a.orp[i] : s;
        int N = 2;
        while (N < len) N <<= 1;
        for (int t = tid; t < N; t += THREADS)
            store(t, t < len ? E::make(sort_key_at<X>(a, xin, i, s, t), (uint32_t)t) : E::pad((uint32_t)t));
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (N >> 1); t += THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int hi = lo | j;
                    const E x = load(lo), y = load(hi);
                    if (y.less(x) == ((lo & k) == 0)) {
                        store(lo, y);
                        store(hi, x);
                    }
                }
                __syncthreads();
            }
        }
        for (int t = tid; t < len; t += THREADS) sort_emit(a, os, len, s + load(t).pos(), t);
        __syncthreads();
    }
}

// keys and payload (the entry's position) of the listed long rows, a workgroup per row
template <class X, class K>
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_long_keys(sort_args a, K *__restrict__ keys,
                                                               uint32_t *__restrict__ pay) {
    const X *__restrict__ xin = (const X *)a.xin;
    const int64_t cnt = min((int64_t)a.stats[2], a.capL);
    for (int64_t b = blockIdx.x; b < cnt; b += gridDim.x) {
        const int64_t s = a.lbeg[b], e = min(a.lend[b], a.nvals), row = a.lrow[b];
        for (int64_t p = s + threadIdx.x; p < e; p += SORT_BLOCK) {
            keys[p] = (K)sort_key_at<X>(a, xin, row, s, p - s);
            pay[p] = (uint32_t)p;
        }
    }
}

__global__ __launch_bounds__(SORT_BLOCK) void k_sort_long_emit(sort_args a, const uint32_t *__restrict__ pay) {
    const int64_t cnt = min((int64_t)a.stats[2], a.capL);
    for (int64_t b = blockIdx.x; b < cnt; b += gridDim.x) {
        const int64_t s = a.lbeg[b], e = min(a.lend[b], a.nvals);
        const int64_t os = a.orp ? a.orp[a.lrow[b]] : s;
        for (int64_t q = s + threadIdx.x; q < e; q += SORT_BLOCK) sort_emit(a, os, e - s, pay[q], (int32_t)(q - s));
    }
}

// sort_method = 1: keys and payload of every entry
template <class X, class K>
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_all_keys(sort_args a, K *__restrict__ keys,
                                                              uint32_t *__restrict__ pay) {
    const X *__restrict__ xin = (const X *)a.xin;
    for (int64_t p = blockIdx.x * (int64_t)SORT_BLOCK + threadIdx.x; p < a.nvals; p += (int64_t)gridDim.x * SORT_BLOCK) {
        keys[p] = (K)sort_key_at<X>(a, xin, 0, p, 0);
        pay[p] = (uint32_t)p;
    }
}

// entry-parallel output of every row: entry q comes from pay[q] (nullptr: from q itself, the
// order an iso matrix already has); its row is upper_bound(rowptr, q) - 1
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_all_emit(sort_args a, const uint32_t *__restrict__ pay) {
    for (int64_t q = blockIdx.x * (int64_t)SORT_BLOCK + threadIdx.x; q < a.nvals; q += (int64_t)gridDim.x * SORT_BLOCK) {
        int64_t lo = 1, hi = a.nrows;  // rowptr[nrows] = nvals > q
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.rowptr[mid] > q) hi = mid;
            else lo = mid + 1;
        }
        const int64_t s = a.rowptr[lo - 1];
        sort_emit(a, s, a.rowptr[lo] - s, pay ? (int64_t)pay[q] : q, (int32_t)(q - s));
    }
}

// rows per class of the last matrix sort, on the device: read only when a counter is asked for
unsigned long long *g_sort_stats = nullptr;

int sort_knob(const char *key, int dflt) {
    const int64_t k = gb_knob(key);
    return k > 0 && k < dflt ? (int)k : dflt;
}

// the cap on a launch's blocks; the knob sort_grid lowers it (tests: few blocks, so that every
// stride loop runs)
int64_t sort_cap(int cap = 8192) { return sort_knob("sort_grid", cap); }

// LT or GT over one type with a BOOL result; returns the operator's type code
int sort_check_op(GrB_BinaryOp op, bool *desc) {
    GB_REQUIRE(op, GrB_NULL_POINTER, "operator is NULL");
    GB_REQUIRE(op->magic == GB_MAGIC, GrB_UNINITIALIZED_OBJECT, "invalid operator");
    GB_REQUIRE(op->xtype && op->ytype && op->ztype && op->ztype->code == GBAMD_T_BOOL &&
                   op->xtype->code == op->ytype->code,
               GrB_DOMAIN_MISMATCH, "sort needs a comparison: BOOL op(T, T)");
    GB_REQUIRE(op->opcode == GBAMD_OP_LT || op->opcode == GBAMD_OP_GT, GrB_NOT_IMPLEMENTED,
               "sort operator must be GrB_LT or GrB_GT");
    *desc = op->opcode == GBAMD_OP_GT;
    return op->xtype->code;
}

void sort_check_perm_type(GB_Obj *P) {
    if (P)
        GB_REQUIRE(P->type->code == GBAMD_T_INT64 || P->type->code == GBAMD_T_UINT64, GrB_DOMAIN_MISMATCH,
                   "the permutation must be GrB_INT64 or GrB_UINT64");
}

// f(X()) with X the key type: sort_rnd for the random order (xcode < 0), else the type of xcode
template <class F>
void sort_with_key(int xcode, F &&f) {
    if (xcode < 0) f(sort_rnd());
    else gb_with_type(xcode, f);
}

template <class K>
void sort_segments(sort_args &a, int xcode, int key_bits, int64_t nseg, const int64_t *beg, const int64_t *end,
                   gb_scratch &s) {
    K *kin = s.get<K>(a.nvals), *kout = s.get<K>(a.nvals);
    uint32_t *pin = s.get<uint32_t>(a.nvals), *pout = s.get<uint32_t>(a.nvals);
    sort_with_key(xcode, [&](auto xv) {
        using X = decltype(xv);
        if (a.all_long)
            hipLaunchKernelGGL((k_sort_all_keys<X, K>), dim3(gb_grid(a.nvals, SORT_BLOCK, sort_cap())),
                               dim3(SORT_BLOCK), 0, gb_stream(), a, kin, pin);
        else
            hipLaunchKernelGGL((k_sort_long_keys<X, K>), dim3(gb_grid(nseg, 1, sort_cap())), dim3(SORT_BLOCK), 0,
                               gb_stream(), a, kin, pin);
    });
    GB_LAUNCH_CHECK();
    size_t tmp = 0;
    GB_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tmp, (const K *)kin, kout, (const uint32_t *)pin, pout,
                                                       (int)a.nvals, (int)nseg, beg, end, 0, key_bits, gb_stream()));
    void *t = s.get<char>(tmp);
    GB_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(t, tmp, (const K *)kin, kout, (const uint32_t *)pin, pout,
                                                       (int)a.nvals, (int)nseg, beg, end, 0, key_bits, gb_stream()));
    if (a.all_long)
        hipLaunchKernelGGL(k_sort_all_emit, dim3(gb_grid(a.nvals, SORT_BLOCK, sort_cap())), dim3(SORT_BLOCK),
                           0, gb_stream(), a, (const uint32_t *)pout);
    else
        hipLaunchKernelGGL(k_sort_long_emit, dim3(gb_grid(nseg, 1, sort_cap())), dim3(SORT_BLOCK), 0, gb_stream(), a,
                           (const uint32_t *)pout);
    GB_LAUNCH_CHECK();
}

// the three row classes over the rows of a (bounds, key type and outputs set by the caller; xcode < 0:
// the random order): the lists, the kernels, and the segmented radix sort of the long rows
void sort_classes(sort_args &a, int xcode, int key_bits, gb_scratch &s) {
    // a row of a class is longer than the class below allows: that bounds the lists
    a.capB = a.all_long ? 0 : std::min(a.nrows, a.nvals / (a.wave_max + 1));
    a.capB2 = a.all_long || a.block_max <= SORT_SMALL_CAP ? 0 : std::min(a.nrows, a.nvals / (SORT_SMALL_CAP + 1));
    a.capL = a.all_long ? 0 : std::min(a.nrows, a.nvals / (a.block_max + 1));
    a.blist = s.get<int64_t>(a.capB);
    a.blist2 = s.get<int64_t>(a.capB2);
    a.lbeg = s.get<int64_t>(3 * a.capL);
    a.lend = a.lbeg + a.capL;
    a.lrow = a.lend + a.capL;
    if (a.capL) gb_memset(a.lbeg, 0, 3 * a.capL * sizeof(int64_t));
    sort_with_key(xcode, [&](auto xv) {
        using X = decltype(xv);
        hipLaunchKernelGGL(k_sort_wave<X>, dim3(gb_sort_grid(a.nrows, 256)), dim3(SORT_BLOCK), 0,
                           gb_stream(), a);
        if (a.capB)
            hipLaunchKernelGGL((k_sort_block<X, SORT_SMALL_CAP, 64>), dim3(gb_grid(a.capB, 1, sort_cap())),
                               dim3(64), 0, gb_stream(), a);
        if (a.capB2)
            hipLaunchKernelGGL((k_sort_block<X, SORT_BLOCK_CAP, SORT_BLOCK>),
                               dim3(gb_grid(a.capB2, 1, sort_cap(4096))), dim3(SORT_BLOCK), 0, gb_stream(), a);
    });
    GB_LAUNCH_CHECK();
    if (a.all_long || a.capL) {
        const int64_t nseg = a.all_long ? a.nrows : a.capL;
        const int64_t *beg = a.all_long ? a.rowptr : a.lbeg, *end = a.all_long ? a.rowptr + 1 : a.lend;
        if (key_bits == 64) sort_segments<uint64_t>(a, xcode, key_bits, nseg, beg, end, s);
        else sort_segments<uint32_t>(a, xcode, key_bits, nseg, beg, end, s);
    }
}

void matrix_sort(GB_Obj *C, GB_Obj *P, GrB_BinaryOp op, GB_Obj *A, const gb_desc &d) {
    GB_REQUIRE(C || P, GrB_NULL_POINTER, "both outputs are NULL");
    bool desc = false;
    const int xcode = sort_check_op(op, &desc);
    GB_REQUIRE(C != P, GrB_NOT_IMPLEMENTED, "C and P are the same matrix");
    sort_check_perm_type(P);
    for (GB_Obj *O : {C, P})
        if (O)
            GB_REQUIRE(O->nrows == A->nrows && gb_ncols_of(O) == gb_ncols_of(A), GrB_DIMENSION_MISMATCH,
                       "output dimensions do not match A");
    gb_csr_view v;
    if (d.tran0) gb_get_csc(v, A);
    else gb_get_csr(v, A);
    const size_t vs = gb_type_size(v.tcode);
    const int64_t nv = v.nvals;
    // hipCUB's segmented sort takes int counts, and whether a row needs it is known on the device only
    GB_REQUIRE(nv < (1LL << 31) && v.nrows < (1LL << 31), GrB_NOT_IMPLEMENTED, "sort of 2^31 or more entries or rows");
    if (!g_sort_stats) g_sort_stats = gb_malloc_n<unsigned long long>(4);
    gb_memset(g_sort_stats, 0, 4 * sizeof(unsigned long long));
    const gb_desc d0;
    if (nv == 0) {
        for (GB_Obj *O : {C, P}) {
            if (!O) continue;
            gb_mat_result T = gb_empty_mat_result(O->nrows, gb_ncols_of(O), O->type->code);
            gb_writeback_matrix(O, T, nullptr, d0, nullptr);
        }
        return;
    }
    // the sorted rows of the view: ranks, values (A's type), columns
    int32_t *ocol = gb_malloc_n<int32_t>(nv);
    void *cvals = C ? gb_malloc((v.iso ? 1 : nv) * vs) : nullptr;
    int64_t *pvals = P ? gb_malloc_n<int64_t>(nv) : nullptr;
    {
        gb_scratch s;
        sort_args a{};
        a.nrows = v.nrows;
        a.nvals = nv;
        a.rowptr = v.rowptr;
        a.colidx = v.colidx;
        a.avals = v.vals;
        a.vs = (int)vs;
        a.oC = v.iso ? nullptr : cvals;
        a.oP = pvals;
        a.ocol = ocol;
        a.stats = g_sort_stats;
        a.m = INT64_MAX;
        if (v.iso) {
            if (C) gb_copy_d2d(cvals, v.vals, vs);
            hipLaunchKernelGGL(k_sort_all_emit, dim3(gb_grid(nv, SORT_BLOCK, sort_cap())), dim3(SORT_BLOCK), 0,
                               gb_stream(), a, (const uint32_t *)nullptr);
            GB_LAUNCH_CHECK();
        } else {
            const int key_bits = 8 * (int)gb_type_size(xcode);
            a.xin = gb_view_vals_as(v, xcode, s);
            a.flip = desc ? (key_bits == 64 ? ~0ull : (1ull << key_bits) - 1) : 0;
            a.wave_max = sort_knob("sort_wave_max", SORT_WAVE_CAP);
            a.block_max = std::max(a.wave_max, sort_knob("sort_block_max", SORT_BLOCK_CAP));
            a.all_long = gb_knob("sort_method") == 1;
            sort_classes(a, xcode, key_bits, s);
        }
    }
    // one result per requested output; under T0 back to CSR through the transpose
    struct out_t {
        GB_Obj *obj;
        void *vals;
        size_t size;
        bool iso;
        int tcode;
    } outs[2] = {{C, cvals, vs, v.iso, v.tcode}, {P, pvals, sizeof(int64_t), false, P ? P->type->code : 0}};
    gb_mat_result T[2];
    for (int k = 0; k < 2; k++) {
        out_t &o = outs[k];
        if (!o.obj) continue;
        T[k].nrows = o.obj->nrows;
        T[k].ncols = gb_ncols_of(o.obj);
        T[k].nvals = nv;
        T[k].tcode = o.tcode;
        T[k].iso = o.iso;
        if (d.tran0) {
            gb_transpose_csr(v.nrows, v.ncols, nv, v.rowptr, ocol, o.vals, o.size, o.iso, &T[k].rowptr, &T[k].colidx,
                             &T[k].vals);
            gb_free(o.vals);
        } else {
            T[k].rowptr = gb_malloc_n<int64_t>(v.nrows + 1);
            gb_copy_d2d(T[k].rowptr, v.rowptr, (v.nrows + 1) * sizeof(int64_t));
            T[k].vals = o.vals;
            if (k == 0 && P) {
                T[k].colidx = gb_malloc_n<int32_t>(nv);
                gb_copy_d2d(T[k].colidx, ocol, nv * sizeof(int32_t));
            } else {
                T[k].colidx = ocol;
                ocol = nullptr;
            }
        }
    }
    gb_free(ocol);
    for (int k = 0; k < 2; k++)
        if (outs[k].obj) gb_writeback_matrix(outs[k].obj, T[k], nullptr, d0, nullptr);
}

// ------------------------------------------------------------------ vectors
__global__ void k_sort_vec_pop(const uint64_t *__restrict__ bits, int64_t n, int64_t nw, int64_t *__restrict__ pop) {
    GB_GRID_LOOP(w, nw) {
        uint64_t b = bits[w];
        if (w == nw - 1 && (n & 63)) b &= (1ull << (n & 63)) - 1;
        pop[w] = __popcll(b);
    }
}

// slot k < nvals: the k-th entry's index and key (X = sort_rnd: the hash of (seed, 0, k); keys =
// nullptr: none); slots from nvals on: the pad
template <class X>
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_vec_compact(int64_t n, const uint64_t *__restrict__ bits,
                                                                 const int64_t *__restrict__ off,
                                                                 const X *__restrict__ xin, bool iso, uint64_t flip,
                                                                 uint64_t padkey, uint64_t seed,
                                                                 uint64_t *__restrict__ keys,
                                                                 int64_t *__restrict__ idx) {
    const int64_t nvals = off[(n + 63) >> 6];
    for (int64_t i = blockIdx.x * (int64_t)SORT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SORT_BLOCK) {
        const uint64_t b = bits[i >> 6];
        if ((b >> (i & 63)) & 1) {
            const int64_t slot = off[i >> 6] + __popcll(b & ((1ull << (i & 63)) - 1));
            idx[slot] = i;
            if constexpr (std::is_same<X, sort_rnd>::value) {
                if (keys) keys[slot] = gb_hash3(seed, 0, (uint64_t)slot);
            } else {
                keys[slot] = sort_key<X>(xin[iso ? 0 : i]) ^ flip;
            }
        }
        if (i >= nvals) {
            idx[i] = 0;
            if (keys) keys[i] = padkey;
        }
    }
}

// dense outputs: w[k] = u[idx[k]], p[k] = idx[k] for k < nvals, zero beyond; bitmaps = nvals ones
__global__ __launch_bounds__(SORT_BLOCK) void k_sort_vec_emit(int64_t n, const int64_t *__restrict__ off,
                                                              const int64_t *__restrict__ idx,
                                                              const void *__restrict__ uvals, int vs, void *wvals,
                                                              int64_t *pvals, uint64_t *wbits, uint64_t *pbits,
                                                              int64_t *wcount, int64_t *pcount) {
    const int64_t nvals = off[(n + 63) >> 6];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (wcount) *wcount = nvals;
        if (pcount) *pcount = nvals;
    }
    for (int64_t k = blockIdx.x * (int64_t)SORT_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * SORT_BLOCK) {
        const bool real = k < nvals;
        const int64_t src = real ? idx[k] : 0;
        if (pvals) pvals[k] = src;
        if (wvals) {
            switch (vs) {
            case 1: ((uint8_t *)wvals)[k] = real ? ((const uint8_t *)uvals)[src] : 0; break;
            case 2: ((uint16_t *)wvals)[k] = real ? ((const uint16_t *)uvals)[src] : 0; break;
            case 4: ((uint32_t *)wvals)[k] = real ? ((const uint32_t *)uvals)[src] : 0; break;
            default: ((uint64_t *)wvals)[k] = real ? ((const uint64_t *)uvals)[src] : 0; break;
            }
        }
        if ((k & 63) == 0) {
            const int64_t left = nvals - k;
            const uint64_t word = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1 : 0;
            if (wbits) wbits[k >> 6] = word;
            if (pbits) pbits[k >> 6] = word;
        }
    }
}

// gb_bitmap_order (gb_internal.h); desc: the descending value order
void bitmap_order(int64_t n, const uint64_t *bits, const void *xin, int xcode, bool iso, bool desc, int mode,
                  uint64_t seed, gb_scratch &s, int64_t **pidx, int64_t **poff) {
    const int64_t nw = gb_words(n);
    int64_t *pop = s.get<int64_t>(nw), *off = s.get<int64_t>(nw + 1);
    const bool sorts = mode == 2 || (mode == 1 && !iso);  // equal keys keep their index order
    uint64_t *keys = sorts || mode == 1 ? s.get<uint64_t>(n) : nullptr;
    int64_t *idx = s.get<int64_t>(n);
    hipLaunchKernelGGL(k_sort_vec_pop, dim3(gb_grid(nw, 256, sort_cap())), dim3(256), 0, gb_stream(), bits, n, nw, pop);
    GB_LAUNCH_CHECK();
    gb_exclusive_scan_i64(pop, off, nw);
    const int key_bits = mode == 1 ? 8 * (int)gb_type_size(xcode) : 64;
    const uint64_t ones = key_bits == 64 ? ~0ull : (1ull << key_bits) - 1;
    sort_with_key(mode == 1 ? xcode : -1, [&](auto xv) {
        using X = decltype(xv);
        hipLaunchKernelGGL(k_sort_vec_compact<X>, dim3(gb_sort_grid(n, SORT_BLOCK)), dim3(SORT_BLOCK), 0, gb_stream(),
                           n, bits, off, (const X *)xin, iso, desc ? ones : 0, ones, seed, keys, idx);
    });
    GB_LAUNCH_CHECK();
    if (sorts) gb_sort_pairs_u64(keys, idx, n, key_bits);
    *pidx = idx;
    *poff = off;
}

void vector_sort(GB_Obj *W, GB_Obj *P, GrB_BinaryOp op, GB_Obj *U) {
    GB_REQUIRE(W || P, GrB_NULL_POINTER, "both outputs are NULL");
    bool desc = false;
    const int xcode = sort_check_op(op, &desc);
    GB_REQUIRE(W != P, GrB_NOT_IMPLEMENTED, "w and p are the same vector");
    sort_check_perm_type(P);
    GB_REQUIRE(gb_ncols_of(U) == 1, GrB_DIMENSION_MISMATCH, "input is not a vector");
    for (GB_Obj *O : {W, P})
        if (O)
            GB_REQUIRE(O->nrows == U->nrows && gb_ncols_of(O) == 1, GrB_DIMENSION_MISMATCH,
                       "output size does not match u");
    gb_bitmap_view uv;
    gb_get_bitmap(uv, U);
    const int64_t n = uv.n, nw = gb_words(n);
    const size_t vs = gb_type_size(uv.tcode);
    gb_vec_result TW, TP;
    if (W) TW = gb_new_vec_result(n, uv.tcode, uv.iso);
    if (P) TP = gb_new_vec_result(n, P->type->code, false);  // INT64 or UINT64: checked above
    if (n == 0) {
        if (W) gb_memset(TW.d_nvals, 0, sizeof(int64_t));
        if (P) gb_memset(TP.d_nvals, 0, sizeof(int64_t));
    } else {
        gb_scratch s;
        int64_t *idx, *off;
        const unsigned grid = gb_grid(n, SORT_BLOCK, sort_cap());
        bitmap_order(n, uv.bits, gb_bitmap_vals_as(uv, xcode, s), xcode, uv.iso, desc, 1, 0, s, &idx, &off);
        if (W && uv.iso) gb_copy_d2d(TW.dense, uv.vals, vs);
        hipLaunchKernelGGL(k_sort_vec_emit, dim3(grid), dim3(SORT_BLOCK), 0, gb_stream(), n, off, idx, uv.vals, (int)vs,
                           W && !uv.iso ? TW.dense : nullptr, P ? (int64_t *)TP.dense : nullptr, W ? TW.bits : nullptr,
                           P ? TP.bits : nullptr, W ? TW.d_nvals : nullptr, P ? TP.d_nvals : nullptr);
        GB_LAUNCH_CHECK();
    }
    const gb_desc d0;
    if (W) gb_writeback_vector(W, TW, nullptr, d0, nullptr, false);
    if (P) gb_writeback_vector(P, TP, nullptr, d0, nullptr, false);
}

}  // namespace

unsigned gb_sort_grid(int64_t items, int64_t per_block) { return gb_grid(items, per_block, sort_cap()); }

void gb_bitmap_order(int64_t n, const uint64_t *bits, const void *xin, int xcode, bool iso, int mode, uint64_t seed,
                     gb_scratch &s, int64_t **idx, int64_t **off) {
    bitmap_order(n, bits, xin, xcode, iso, false, mode, seed, s, idx, off);
}

void gb_rank_rows(const gb_rank_job &j) {
    GB_REQUIRE(j.nvals < (1LL << 31) && j.nrows < (1LL << 31), GrB_NOT_IMPLEMENTED,
               "selection by value or at random among 2^31 or more entries or rows");
    gb_scratch s;
    sort_args a{};
    a.nrows = j.nrows;
    a.nvals = j.nvals;
    a.rowptr = j.rowptr;
    a.colidx = j.colidx;
    a.xin = j.xin;
    a.avals = j.avals;
    a.vs = j.vs;
    a.oC = j.oC;
    a.oP = j.oP;
    a.ocol = j.ocol;
    a.stats = j.stats;
    a.orp = j.orp;
    a.m = j.m;
    a.far = j.far;
    a.reverse = j.reverse;
    a.keep = j.keep;
    a.seed = j.seed;
    a.wave_max = j.wave_max > 0 ? std::min(j.wave_max, SORT_WAVE_CAP) : sort_knob("sort_wave_max", SORT_WAVE_CAP);
    a.block_max = j.block_max > 0 ? std::min(j.block_max, SORT_BLOCK_CAP) : sort_knob("sort_block_max", SORT_BLOCK_CAP);
    a.block_max = std::max(a.wave_max, a.block_max);
    sort_classes(a, j.random ? -1 : j.xcode, j.random ? 64 : 8 * (int)gb_type_size(j.xcode), s);
}

bool gb_sort_stat(const char *key, int64_t *value) {
    static const char *names[3] = {"stat_sort_rows_wave", "stat_sort_rows_block", "stat_sort_rows_long"};
    for (int k = 0; k < 3; k++) {
        if (strcmp(key, names[k])) continue;
        *value = g_sort_stats ? gb_read_i64((const int64_t *)g_sort_stats + k) : 0;
        if (k == 1 && g_sort_stats) *value += gb_read_i64((const int64_t *)g_sort_stats + 3);  // both workgroup sizes
        return true;
    }
    // the class bounds read back as their defaults while unset
    for (const auto &kd : {std::make_pair("sort_wave_max", SORT_WAVE_CAP), std::make_pair("sort_block_max", SORT_BLOCK_CAP)}) {
        if (strcmp(key, kd.first)) continue;
        *value = sort_knob(kd.first, kd.second);
        return true;
    }
    return false;
}

extern "C" {

GrB_Info GxB_Matrix_sort(GrB_Matrix C, GrB_Matrix P, GrB_BinaryOp op, const GrB_Matrix A, const GrB_Descriptor desc) {
    return gb_api(OBJ(C ? C : P), [&] {
        GB_REQUIRE(A, GrB_NULL_POINTER, "A is NULL");
        matrix_sort(gb_obj_check(C, true), gb_obj_check(P, true), op, gb_obj_check(A), gb_read_desc(desc));
    });
}

GrB_Info GxB_Vector_sort(GrB_Vector w, GrB_Vector p, GrB_BinaryOp op, const GrB_Vector u, const GrB_Descriptor desc) {
    return gb_api(OBJ(w ? w : p), [&] {
        GB_REQUIRE(u, GrB_NULL_POINTER, "u is NULL");
        gb_read_desc(desc);
        vector_sort(gb_obj_check(w, true), gb_obj_check(p, true), op, gb_obj_check(u));
    });
}

}  // extern "C"
