// gb_spmv_iso.hip -- the BFS path: every masked SpMV whose result is iso
// (gb_spmv_result_iso: lor_land, any_pair, min_first over an iso operand, ...).
// Only presence is computed; the one value is mult(a0, u0), evaluated on the
// device from the operator and type codes (gb_iso_eval).  Nothing here is a
// template over the semiring: gb_spmv (gb_mxv.hip) calls gb_spmv_iso directly.
//
// One launch per call by default:
//   k_iso_work  picks the direction, does it and finishes the result (count,
//               next-frontier edge hint, iso value, host mailbox) --
//     push (top-down): each frontier row of the other orientation of A' sets
//       the bits of its unmasked targets with atomicOr; a wave spreads the
//       rows of one frontier word over its lanes; rows longer than H are cut
//       into H-edge chunks (a table cached on the matrix) spread over waves;
//     pull (bottom-up): one lane per output row, stop at the first k in u.
//   The direction comes from the frontier's edge-count hint (left on u by the
//   launch that produced it; Beamer's rule m_f * alpha < m_u on the device),
//   from the host when the frontier is a pending root or provably small, and is
//   pull when there is no push orientation.
//   k_dir_prep  runs before k_iso_work only when none of these holds (a frontier
//               without a usable hint, no zeroed spare output, knob host_dir 1):
//               frontier edge count m_f (grid-wide sum; the block completing it
//               applies Beamer's rule), zeroed output.
// No host round trip is needed for the choice.
#include <mutex>

#include "gb_dispatch.cuh"
#include "gb_internal.h"

// Direction state words (gb_state.h, GB_DIR_STATE_OFFSET; ST_PUSHES apart, zero between calls
// except ST_PUSH, which every prep rewrites):
//   [ST_PUSH]     chosen direction: 1 push, 0 pull (written by the last prep block)
//   [ST_PUSHES]   launches of k_iso_work that pushed, since the process began (a running
//                 count, never reset: GxB_Global_get_int "stat_iso_push_launches" -- what the
//                 device chose is not otherwise visible to the host, the results being the same)
enum { ST_PUSH = 0, ST_PUSHES = 1 };
int64_t gb_iso_push_launches() {
    unsigned long long c = 0;
    GB_HIP(hipStreamSynchronize(gb_stream()));
    GB_HIP(hipMemcpy(&c, gb_device_state() + GB_DIR_STATE_OFFSET + ST_PUSHES, sizeof(c), hipMemcpyDeviceToHost));
    return (int64_t)c;
}
#define PULL_U 4  // bitmap words per wave step (independent loads in flight)

struct gb_dir_rule {
    const int64_t *mask_count;  // device count of set mask bits (nullptr: unknown)
    const int64_t *extra_count; // entries a fused assign adds to the mask (upper bound; nullptr: none)
    bool mcomp;
    int64_t n_out, nnz, alpha;
    int force_push;
};

// Beamer's rule: push while the frontier's edges m_f (times alpha) are fewer
// than the edges the pull would examine, estimated as open rows x average degree
__device__ __forceinline__ bool gb_dir_decide(long long mf, const gb_dir_rule &rule) {
    int64_t open = rule.n_out;  // rows the pull kernel would visit
    if (rule.mask_count) {
        int64_t mc = *rule.mask_count;
        if (rule.extra_count) mc += *rule.extra_count;
        if (mc > rule.n_out) mc = rule.n_out;
        open = rule.mcomp ? (rule.n_out - mc) : mc;
    }
    const double avg = rule.n_out ? (double)rule.nnz / (double)rule.n_out : 0.0;
    return rule.force_push || ((double)mf * (double)rule.alpha < (double)open * avg);
}

// Prep: m_f = edges of the frontier in the push orientation (one lane per
// frontier bit); zeroes the output bitmap and count (the iso value is
// k_iso_work's).  The block that completes the grid-wide sum of m_f applies
// Beamer's rule m_f * alpha < m_u and stores the direction.
__global__ __launch_bounds__(SPMV_BLOCK) void k_dir_prep(
    const uint64_t *__restrict__ ubits, int64_t nwords_u, const int64_t *__restrict__ prow,
    unsigned long long *__restrict__ gst, unsigned long long *__restrict__ dst,
    uint64_t *__restrict__ tbits, int64_t nwords_out, unsigned long long *__restrict__ tcount, gb_dir_rule rule) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    long long mf = 0;
    // 16 frontier words per wave step (lanes 0-15 load them); the non-zero ones
    // are expanded one lane per bit, four words at a time
    for (int64_t base = wave * 16; base < nwords_u; base += nwaves * 16) {
        const int64_t wl = base + (lane & 15);
        const uint64_t mine = wl < nwords_u ? ubits[wl] : 0;
        unsigned long long nz = __ballot(mine != 0) & 0xFFFFULL;
        while (nz) {
            int64_t deg[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                deg[u] = 0;
                if (nz) {
                    const int l = __ffsll(nz) - 1;
                    nz &= nz - 1;
                    const uint64_t word = __shfl(mine, l, 64);
                    if ((word >> lane) & 1ULL) {
                        const int64_t k = ((base + l) << 6) + lane;
                        deg[u] = prow[k + 1] - prow[k];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) mf += deg[u];
        }
    }
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t w = tid; w < nwords_out; w += (int64_t)gridDim.x * blockDim.x) tbits[w] = 0;
    if (tid == 0) *tcount = 0;
    long long total;
    if (gb_grid_sum(mf, gst, &total)) dst[ST_PUSH] = gb_dir_decide(total, rule) ? 1ULL : 0ULL;
}

// set the output bits of up to W targets per lane (unmasked, not yet set);
// returns how many bits this lane turned on.  hlen (nullptr: no hint): the row lengths the
// next-frontier hint sums over the added vertices (gb_hub_sections::rowlen), read after the
// atomics, all at once
template <int W>
__device__ __forceinline__ long long gb_push_targets(const int32_t (&j)[W], bool (&ok)[W],
                                                     const uint64_t *__restrict__ mbits, bool mcomp,
                                                     unsigned long long *__restrict__ tbits,
                                                     const uint32_t *__restrict__ hlen, long long &mfn,
                                                     const uint64_t *__restrict__ qbits, bool serial = false,
                                                     int64_t qroot = -1) {
    uint32_t cur[W];  // the 32-bit half of the output word that holds the target's bit
    const uint32_t *t32 = reinterpret_cast<const uint32_t *>(tbits);
    if (serial) {  // diagnostics (iso_dbg 128): the round-4 order, each read behind the one before
        if (mbits) {
#pragma unroll
            for (int u = 0; u < W; u++)
                if (ok[u]) ok[u] = (gb_bit(mbits, j[u]) || (qbits && gb_bit(qbits, j[u]))) != mcomp;
        }
#pragma unroll
        for (int u = 0; u < W; u++) cur[u] = ok[u] ? t32[j[u] >> 5] : ~0u;
    } else {
        // the mask words (w's and the fused stamp's q) and the output word of every target are
        // read at once: one round trip instead of three dependent ones.  Only the halves that
        // hold the targets' bits are read (half the registers)
        const uint32_t *m32 = reinterpret_cast<const uint32_t *>(mbits);
        const uint32_t *q32 = reinterpret_cast<const uint32_t *>(qbits);
        uint32_t mw[W], qw[W];
#pragma unroll
        for (int u = 0; u < W; u++) {
            mw[u] = qw[u] = 0;
            cur[u] = ~0u;
            if (ok[u]) {
                if (mbits) mw[u] = m32[j[u] >> 5];
                if (mbits && qbits) qw[u] = q32[j[u] >> 5];
                cur[u] = t32[j[u] >> 5];
            }
        }
        if (mbits) {
            // qroot: the fused stamp's frontier is one pending vertex (gb_push_root), not q's bits
#pragma unroll
            for (int u = 0; u < W; u++)
                if (ok[u]) ok[u] = (((((mw[u] | qw[u]) >> (j[u] & 31)) & 1u) != 0) || j[u] == qroot) != mcomp;
        }
    }
    // every atomic of the step is issued before the first result is looked at (a result tested
    // where its atomic is issued makes each one wait for the one before: W round trips).  The
    // atomics too go to the 32-bit halves; within a launch nothing else writes the output words
    unsigned int *t32w = reinterpret_cast<unsigned int *>(tbits);
    uint32_t old[W];
    bool won[W];  // first: the atomic is tried
    // (the words read above are all tested before the first atomic: a read's result used
    // between two atomics under conditions waits for the atomic before it too.  old starts as
    // that word, not a constant: the compiler moves a test of "constant or the atomic's
    // result" up to the atomic, and its wait with it)
#pragma unroll
    for (int u = 0; u < W; u++) {
        old[u] = cur[u];
        won[u] = ok[u] && !((cur[u] >> (j[u] & 31)) & 1u);
    }
#pragma unroll
    for (int u = 0; u < W; u++)
        if (won[u]) old[u] = atomicOr(&t32w[j[u] >> 5], 1u << (j[u] & 31));
#pragma unroll
    for (int u = 0; u < W; u++) won[u] = won[u] && !((old[u] >> (j[u] & 31)) & 1u);
    long long added = 0;
#pragma unroll
    for (int u = 0; u < W; u++) added += won[u] ? 1 : 0;
    // edges of the next frontier
    if (hlen) {
        // (every lane reads, element 0 where nothing was added: the sum of "0 or a load under
        // a condition" is moved up to the load by the compiler, and each load then waited for)
        uint32_t dl[W];
#pragma unroll
        for (int u = 0; u < W; u++) dl[u] = hlen[won[u] ? j[u] : 0];
#pragma unroll
        for (int u = 0; u < W; u++) mfn += won[u] ? dl[u] : 0u;
    }
    return added;
}

// ------------------------------------------------ wave-level segment lists (LDS)
// A wave gathers up to WL_MAX row segments (start, length) into its own LDS
// area, takes a prefix sum of the lengths and then walks the concatenated
// edges 256 at a time, four independent loads per lane; a lane finds the
// segment of its edge by binary search over the prefix.  This keeps every lane
// busy whatever the mix of row lengths (no lane-per-row tail, no wave per row).
#define WL_MAX 256
struct gb_wlist {
    int64_t p[WL_MAX];    // next edge position of the segment
    int32_t rem[WL_MAX];  // edges left in the row
    int32_t pref[WL_MAX]; // inclusive prefix of this round's lengths
    int16_t id[WL_MAX];   // u * 64 + lane of the row (pull)
    int8_t hit[WL_MAX];   // a k present in u was found this round
    unsigned long long hitw[PULL_U];  // pull: rows of the unit's words found through the list
};

// this round takes min(rem[i], cap) edges of segment i; hit[i] = 0; pref = inclusive
// prefix of the taken lengths; returns the total
__device__ __forceinline__ int gb_wlist_round(gb_wlist &L, int n, int cap, int lane) {
    int v[4], sum = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = lane * 4 + t;
        v[t] = 0;
        if (i < n) {
            v[t] = L.rem[i] < cap ? L.rem[i] : cap;
            L.hit[i] = 0;
        }
        sum += v[t];
    }
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    int run = incl - sum;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = lane * 4 + t;
        run += v[t];
        if (i < n) L.pref[i] = run;
    }
    gb_wave_sync();
    return __shfl(incl, 63, 64);
}

// start of segment i's edges in the concatenated stream
__device__ __forceinline__ int gb_wlist_start(const gb_wlist &L, int i) { return i ? L.pref[i - 1] : 0; }

// segment of concatenated edge e: first i with pref[i] > e (n <= WL_MAX)
__device__ __forceinline__ int gb_wlist_find(const gb_wlist &L, int n, int e) {
    int lo = 0;
#pragma unroll
    for (int st = WL_MAX / 2; st > 0; st >>= 1)
        if (lo + st <= n && L.pref[lo + st - 1] <= e) lo += st;
    return lo;
}

// pull: after a round's walk, rows that hit set their bit in hitw; the survivors (no hit, edges
// left) are compacted in place (chunks of 64, in order); returns how many survive
__device__ __forceinline__ int gb_wlist_survivors(gb_wlist &L, int n, int lane, unsigned long long lt) {
    int m = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        bool alive = false, hit = false;
        int64_t np = 0;
        int32_t nr = 0;
        int16_t id = 0;
        if (i < n) {
            const int32_t taken = L.pref[i] - gb_wlist_start(L, i);
            hit = L.hit[i] != 0;
            id = L.id[i];
            np = L.p[i] + taken;
            nr = L.rem[i] - taken;
            alive = !hit && nr > 0;
        }
        if (hit) atomicOr(&L.hitw[id >> 6], 1ULL << (id & 63));
        const unsigned long long ab = __ballot(alive);
        gb_wave_sync();
        if (alive) {
            const int j = m + __popcll(ab & lt);
            L.p[j] = np;
            L.rem[j] = nr;
            L.id[j] = id;
        }
        m += __popcll(ab);
        gb_wave_sync();
    }
    return m;
}

// The fused assign (gb_asg) for the 4 words w0..w0+3 of q (lanes 0-3 hold word
// w0 + (lane & 3) in qw): w's presence words |= q, w's value at each q bit = x
// (one lane per position: coalesced stores); returns the entries added to w.
struct gb_asg_dev {
    uint64_t *bits;
    void *vals;
    int size;
    unsigned long long x;
};
__device__ __forceinline__ void gb_store_sized(void *base, int64_t i, int size, unsigned long long x) {
    switch (size) {
    case 1: ((uint8_t *)base)[i] = (uint8_t)x; break;
    case 2: ((uint16_t *)base)[i] = (uint16_t)x; break;
    case 4: ((uint32_t *)base)[i] = (uint32_t)x; break;
    default: ((unsigned long long *)base)[i] = x; break;
    }
}
// cpre: w's word already read by the caller (nullptr: read it here)
__device__ __forceinline__ long long gb_asg_words(const gb_asg_dev &g, int64_t w0, int64_t nwords, uint64_t qw,
                                                 int lane, const uint64_t *cpre = nullptr) {
    long long added = 0;
    const int64_t wl = w0 + (lane & 3);
    if (lane < 4 && wl < nwords && qw) {
        const uint64_t c = cpre ? *cpre : g.bits[wl], nwd = c | qw;
        if (nwd != c) g.bits[wl] = nwd;
        added = (long long)__popcll(nwd) - (long long)__popcll(c);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint64_t word = __shfl(qw, u, 64);
        if ((word >> lane) & 1ULL) gb_store_sized(g.vals, ((w0 + u) << 6) + lane, g.size, g.x);
    }
    return added;
}

// Push (top-down).  First the matrix's hub chunks (rows longer than H cut into
// H-edge pieces, a static table that holds each piece's row and bounds; a wave
// tests 16 strided entries against the frontier at once and expands the hits,
// 512 edges a step).  Then the frontier words, 4 per wave step: the rows of
// their frontier vertices (at most H edges each) go into the wave's segment
// list and are walked as one edge stream.  The row bounds of the first step's
// vertices (and the fused stamp's word) are read in the round trip of the hub
// entries' frontier-bit probes, not after the hub pieces.
__device__ __forceinline__ long long gb_push_phase(int64_t nwords_u, const uint64_t *__restrict__ ubits,
                                                  const int64_t *__restrict__ prow, const int32_t *__restrict__ pcol,
                                                  const int32_t *__restrict__ hubs, int64_t nhubs, int64_t H,
                                                  const uint64_t *__restrict__ mbits, bool mcomp,
                                                  unsigned long long *__restrict__ tbits, gb_wlist &L,
                                                  const uint32_t *__restrict__ hlen, long long &mfn,
                                                  const uint64_t *__restrict__ qbits, const gb_asg_dev &g,
                                                  long long &adelta, bool serial = false, bool prefetch = true,
                                                  bool defer = false) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    const gb_hub_sections sec = gb_hub_sections_of(hubs, nhubs);
    long long added = 0;
    // the frontier words of this wave's first 16 steps, loaded before the hub chunks (round 5):
    // lane l holds step l / 4's word l % 4, so a small frontier's scan costs one load round trip
    // (overlapped with the hub test's) instead of one per step -- with one wave of workgroups a
    // wave takes nwords / (4 * waves) steps, 4 at s22
    uint64_t pre = 0;
    {
        const int64_t wl = wave * 4 + (int64_t)(lane >> 2) * nwaves * 4 + (lane & 3);
        if (wl < nwords_u) pre = ubits[wl];
    }
    // hub chunks: lane l of wave w tests table entry w + l * nwaves (a hub's consecutive
    // chunks land on different waves).  An entry's row and its piece's bounds come in one
    // round trip -- the first sweep's with the frontier words above
    int hk = -1, hl = 0;  // the tested piece's row (-1: none) and length
    int64_t hp = 0;        // its first edge
    uint64_t hw;  // the frontier word of the entry's row
    auto hub_entry = [&](int64_t base) {
        const int64_t h = base + (int64_t)lane * nwaves;
        hk = -1;
        if (lane < 16 && h < nhubs) {
            const gb_hub_piece pc = sec.piece[h];  // one 16-byte load
            hk = pc.row;
            hl = pc.len;
            hp = pc.pos;
        }
    };
    if (wave < nhubs) hub_entry(wave);
    // one step's frontier rows: their bounds and the fused stamp's word, all loads at once ...
    auto rows_load = [&](int64_t w0, uint64_t mine, int64_t (&p0)[4], int64_t (&d)[4], uint64_t &cw) {
        const int64_t wl = w0 + (lane & 3);
        cw = 0;
        if (qbits && lane < 4 && wl < nwords_u && mine) cw = g.bits[wl];
        int64_t p1[4];  // the lengths are taken after the last load is issued, or each load waits
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t word = __shfl(mine, u, 64);
            p0[u] = p1[u] = 0;
            if ((word >> lane) & 1ULL) {
                const int64_t k = ((w0 + u) << 6) + lane;
                p0[u] = prow[k];
                p1[u] = prow[k + 1];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) d[u] = p1[u] - p0[u];
    };
    // the wave's segment list walked as one edge stream, then emptied
    int n = 0;
    auto flush = [&]() {
        gb_wave_sync();
        const int total = gb_wlist_round(L, n, 1 << 30, lane);
        for (int e0 = 0; e0 < total; e0 += 256) {
            int32_t j[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = e0 + lane + 64 * u;
                ok[u] = e < total;
                j[u] = 0;
                if (ok[u]) {
                    const int s = gb_wlist_find(L, n, e);
                    j[u] = pcol[L.p[s] + (e - gb_wlist_start(L, s))];
                }
            }
            added += gb_push_targets<4>(j, ok, mbits, mcomp, tbits, hlen, mfn, qbits, serial);
        }
        gb_wave_sync();
        n = 0;
    };
    // ... then the stamp of the step's words, and its rows (hubs apart) appended to the list
    auto rows_add = [&](int64_t w0, uint64_t mine, const int64_t (&p0)[4], const int64_t (&d)[4], uint64_t cw) {
        if (qbits) adelta += gb_asg_words(g, w0, nwords_u, mine, lane, &cw);
        unsigned long long bb[4];
        int add = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            bb[u] = __ballot(d[u] > 0 && d[u] <= H);  // hubs: done by their chunks
            add += __popcll(bb[u]);
        }
        if (!add) return;
        if (n + add > WL_MAX) flush();  // a step has at most 256 rows: it fits an empty list
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if ((bb[u] >> lane) & 1ULL) {
                const int i = n + __popcll(bb[u] & lt);
                L.p[i] = p0[u];
                L.rem[i] = (int32_t)d[u];
            }
            n += __popcll(bb[u]);
        }
    };
    // the first sweep's frontier-bit probes go out with the bounds of the first step's rows
    // (every lane reads a word, word 0 without an entry: a load under a condition whose result
    // is tested at once is waited for where it is issued)
    int step = 0;
    int64_t w0 = wave * 4;
    bool act;
    {
        const bool first = prefetch && w0 < nwords_u;
        const uint64_t mine = first ? __shfl(pre, lane & 3, 64) : 0;
        int64_t p0[4], d[4];
        uint64_t cw;
        const bool any = __ballot(mine != 0) != 0;
        // (the probe is issued after the wait for the frontier words: issued before it, that
        // wait -- which cannot tell how many loads under conditions are in flight -- would
        // take the probe in, and the rows' bounds would go out a round trip later)
        __builtin_amdgcn_sched_barrier(0);
        hw = ubits[(hk >= 0 ? hk : 0) >> 6];
        if (any) rows_load(w0, mine, p0, d, cw);
        act = hk >= 0 && ((hw >> (hk & 63)) & 1ULL);
        if (any) rows_add(w0, mine, p0, d, cw);
        if (first) {
            step = 1;
            w0 += nwaves * 4;
        }
    }
    // hits are expanded in turn, 512 edges a step: 8 columns per lane, then all the targets'
    // words, then the atomics
    for (int64_t base = wave; base < nhubs;) {
        unsigned long long b = __ballot(act);
        while (b) {
            const int l = __ffsll(b) - 1;
            b &= b - 1;
            const int64_t pp = __shfl(hp, l, 64);
            const int ln = __shfl(hl, l, 64);
            for (int e0 = lane; e0 < ln; e0 += 512) {
                int32_t j[8];
                bool ok[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    ok[u] = e0 + 64 * u < ln;
                    j[u] = ok[u] ? pcol[pp + e0 + 64 * u] : 0;
                }
                added += gb_push_targets<8>(j, ok, mbits, mcomp, tbits, hlen, mfn, qbits, serial);
            }
        }
        base += nwaves * 16;
        if (base >= nhubs) break;
        hub_entry(base);
        hw = ubits[(hk >= 0 ? hk : 0) >> 6];
        act = hk >= 0 && ((hw >> (hk & 63)) & 1ULL);
    }
    if (n && !defer) flush();
    // frontier words, 4 per wave step (lanes 0-3 load them; the first 16 steps' came above).
    // defer (knob iso_pack): the rows of successive steps pile up in the list, which is walked
    // only when the next step's rows would not fit or the words are exhausted -- one chain of
    // edge / mask / output reads for a sparse frontier's few rows per step instead of one per step
    for (; w0 < nwords_u; w0 += nwaves * 4, step++) {
        const int64_t wl = w0 + (lane & 3);
        uint64_t mine;
        if (prefetch && step < 16) {
            mine = __shfl(pre, (step << 2) | (lane & 3), 64);
        } else {
            mine = wl < nwords_u ? ubits[wl] : 0;
        }
        if (!__ballot(mine != 0)) continue;
        int64_t p0[4], d[4];
        uint64_t cw;
        rows_load(w0, mine, p0, d, cw);
        rows_add(w0, mine, p0, d, cw);
        if (n && !defer) flush();
    }
    if (n) flush();
    return added;
}

// Push from a single pending vertex (the BFS root, gb_bfs_loop.hip gb_root_try_defer): the host knows
// the frontier is {root}, so the kernel neither tests the hub table against the frontier nor
// scans its bitmap words (which do not hold the root) -- the root's edges are spread over the
// whole grid, 4 per lane per step, and block 0 carries out the fused stamp v<q> = x for it.
// Replaces the single-thread set launch and the first level's two scan round trips.
__device__ __forceinline__ long long gb_push_root(int64_t root, const int64_t *__restrict__ prow,
                                                 const int32_t *__restrict__ pcol,
                                                 const uint64_t *__restrict__ mbits, bool mcomp,
                                                 unsigned long long *__restrict__ tbits,
                                                 const uint32_t *__restrict__ hlen, long long &mfn,
                                                 bool stamp, const gb_asg_dev &g, long long &adelta) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (stamp && blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long m = 1ULL << (root & 63);
        const unsigned long long old = atomicOr((unsigned long long *)&g.bits[root >> 6], m);
        gb_store_sized(g.vals, root, g.size, g.x);
        if (!(old & m)) adelta += 1;
    }
    const int64_t p0 = prow[root], p1 = prow[root + 1];
    long long added = 0;
    for (int64_t p = p0 + wave * 256 + lane; p < p1; p += nwaves * 256) {
        int32_t j[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ok[u] = p + 64 * u < p1;
            j[u] = ok[u] ? pcol[p + 64 * u] : 0;
        }
        added += gb_push_targets<4>(j, ok, mbits, mcomp, tbits, hlen, mfn, nullptr, false, stamp ? root : -1);
    }
    return added;
}

// The pull heads and pdeg hold one record per non-empty row, indexed by the row's rank among
// them: the prefix of the row's bitmap word (ne_rank, loaded with the step's other control
// words) + the non-empty rows below it in the word (rw: the word of rows_nonempty).
__device__ __forceinline__ uint32_t gb_ne_rank(uint32_t prefix, uint64_t rw, int bit) {
    return prefix + (uint32_t)__popcll(rw & ((1ULL << bit) - 1));
}
// lane l's 64-bit x on every lane (l wave-uniform)
__device__ __forceinline__ uint64_t gb_readlane64(uint64_t x, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// The pull-head probes of a wave step in two rounds, each with every load in flight at once:
// the first head of every open row, then the other three for the rows it missed (a
// short-circuit test makes each probe wait for the one before it: up to 16 dependent
// frontier reads per wave step).  hv: a row's heads (-1: none); found[u]: one of them is in u.
__device__ __forceinline__ void gb_pull_probe_heads(const int4 (&hv)[PULL_U], const uint64_t *__restrict__ ubits,
                                                    bool (&found)[PULL_U]) {
    const uint32_t *ub32 = reinterpret_cast<const uint32_t *>(ubits);
    uint32_t w1[PULL_U];
#pragma unroll
    for (int u = 0; u < PULL_U; u++) {
        w1[u] = 0;
        if (hv[u].x >= 0) w1[u] = ub32[hv[u].x >> 5];
    }
#pragma unroll
    for (int u = 0; u < PULL_U; u++) found[u] = hv[u].x >= 0 && ((w1[u] >> (hv[u].x & 31)) & 1u);
    uint32_t wy[PULL_U], wz[PULL_U], ww[PULL_U];
#pragma unroll
    for (int u = 0; u < PULL_U; u++) {
        wy[u] = wz[u] = ww[u] = 0;
        if (!found[u]) {
            if (hv[u].y >= 0) wy[u] = ub32[hv[u].y >> 5];
            if (hv[u].z >= 0) wz[u] = ub32[hv[u].z >> 5];
            if (hv[u].w >= 0) ww[u] = ub32[hv[u].w >> 5];
        }
    }
#pragma unroll
    for (int u = 0; u < PULL_U; u++)
        found[u] = found[u] || (hv[u].y >= 0 && ((wy[u] >> (hv[u].y & 31)) & 1u)) ||
                   (hv[u].z >= 0 && ((wz[u] >> (hv[u].z & 31)) & 1u)) ||
                   (hv[u].w >= 0 && ((ww[u] >> (hv[u].w & 31)) & 1u));
}

// The pull's segment list (n rows, L.hitw zeroed) walked as one edge stream in rounds until no
// row survives: at most `cap` edges per row per round, cap doubling from cap0; a row that finds a
// k present in u leaves the list with its bit set in L.hitw (visible to the wave on return).
__device__ __forceinline__ void gb_wlist_walk_pull(gb_wlist &L, int n, int cap0, const int32_t *__restrict__ colidx,
                                                   const uint64_t *__restrict__ ubits) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ULL << lane) - 1;
    int cap = cap0;
    while (n) {
        gb_wave_sync();
        const int total = gb_wlist_round(L, n, cap, lane);
        for (int e0 = 0; e0 < total; e0 += 256) {
            int k[4], s[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int e = e0 + lane + 64 * u;
                ok[u] = e < total;
                s[u] = 0;
                k[u] = 0;
                if (ok[u]) {
                    s[u] = gb_wlist_find(L, n, e);
                    k[u] = colidx[L.p[s[u]] + (e - gb_wlist_start(L, s[u]))];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (ok[u] && gb_bit(ubits, k[u])) L.hit[s[u]] = 1;
        }
        gb_wave_sync();
        n = gb_wlist_survivors(L, n, lane, lt);
        cap = cap < (1 << 20) ? cap * 2 : cap;
    }
    gb_wave_sync();
}

// Pull (bottom-up) for iso results: only presence is computed.  A wave takes
// PULL_U 64-row bitmap words at a time, one lane per row of each: a lane walks
// its own rows four edges a step (neighbouring rows are neighbouring in colidx,
// so the loads coalesce), stopping at the first k present in u.  Rows still
// open after 8 edges go into the wave's segment list and are walked as one
// edge stream in rounds (at most `cap` edges per row per round, cap doubling),
// dropping the rows that found a k after each round.
__device__ __forceinline__ long long gb_pull_iso_phase(int64_t nrows, const int64_t *__restrict__ rowptr,
                                                      const int32_t *__restrict__ colidx,
                                                      const uint64_t *__restrict__ ubits,
                                                      const uint64_t *__restrict__ mbits, bool mcomp,
                                                      uint64_t *__restrict__ tbits, gb_wlist &L,
                                                      const int64_t *__restrict__ hprow, long long &mfn,
                                                      int p1_steps, int cap0, const uint64_t *__restrict__ rne,
                                                      const uint64_t *__restrict__ qbits, const gb_asg_dev &g,
                                                      long long &adelta, int dbg = 0,
                                                      const int32_t *__restrict__ ph = nullptr,
                                                      const uint32_t *__restrict__ pdeg = nullptr,
                                                      const uint32_t *__restrict__ nrk = nullptr) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nwords = (nrows + 63) >> 6;
    const uint64_t tail = (nrows & 63) ? ((1ULL << (nrows & 63)) - 1) : ~0ULL;
    const unsigned long long lt = (1ULL << lane) - 1;
    long long cnt = 0;
    for (int64_t w0 = wave * PULL_U; w0 < nwords; w0 += nwaves * PULL_U) {
        const int64_t wl = w0 + (lane & (PULL_U - 1));
        const bool inr = wl < nwords;
        // the step's words read together (the stamp's q, the mask, the rows with entries): the
        // stamp's store no longer orders the mask read behind it
        const uint64_t qw = (qbits && inr) ? qbits[wl] : 0;
        const uint64_t mw = (mbits && inr) ? mbits[wl] : 0;
        const uint64_t rw = (rne && inr) ? rne[wl] : ~0ULL;
        const uint32_t nr = (ph && inr) ? nrk[wl] : 0;  // the heads' rank prefix: the same round trip
        uint64_t mine = ~0ULL;
        if (qbits) {  // fused assign: w |= q; the mask is w's structure after it
            adelta += gb_asg_words(g, w0, nwords, qw, lane, g.bits == mbits ? &mw : nullptr);
            if (mbits) mine = inr ? (mcomp ? ~(mw | qw) : (mw | qw)) : 0;
        } else if (mbits) {
            mine = inr ? (mcomp ? ~mw : mw) : 0;
        }
        if (rne && inr) mine &= rw;  // rows without entries produce nothing
        if (wl == nwords - 1) mine &= tail;
        if (wl >= nwords) mine = 0;
        if (!__ballot(mine != 0)) {  // nothing open in these words
            if (lane < PULL_U && wl < nwords) tbits[wl] = 0;
            continue;
        }
        bool live[PULL_U], found[PULL_U];
        int64_t p[PULL_U], p1[PULL_U];
        int64_t dg[PULL_U];
#pragma unroll
        for (int u = 0; u < PULL_U; u++) {
            live[u] = (__shfl(mine, u, 64) >> lane) & 1ULL;
            found[u] = false;
        }
        if (ph) {
            // pull heads: each open row first tests its best-connected neighbours (one coalesced
            // 16-byte load per row); rows they settle, and rows of at most 4 entries, never read
            // their bounds or edges -- the dependent row-pointer / edge round trips are left to
            // the long rows that found nothing
            int4 hv[PULL_U];
            uint32_t rk[PULL_U];  // the rows' records (an open row has entries: its bit is set in rw)
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                rk[u] = gb_ne_rank((uint32_t)__builtin_amdgcn_readlane((int)nr, u), gb_readlane64(rw, u), lane);
                hv[u] = make_int4(-1, -1, -1, -1);
                if (live[u]) hv[u] = reinterpret_cast<const int4 *>(ph)[rk[u]];
            }
            if (dbg & 128) {  // diagnostics: the round-4 short-circuit probes (A/B)
#pragma unroll
                for (int u = 0; u < PULL_U; u++)
                    found[u] = (hv[u].x >= 0 && gb_bit(ubits, hv[u].x)) ||
                               (hv[u].y >= 0 && gb_bit(ubits, hv[u].y)) ||
                               (hv[u].z >= 0 && gb_bit(ubits, hv[u].z)) ||
                               (hv[u].w >= 0 && gb_bit(ubits, hv[u].w));
            } else {
                gb_pull_probe_heads(hv, ubits, found);
            }
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                const int64_t r = ((w0 + u) << 6) + lane;
                p[u] = p1[u] = 0;
                if (live[u] && !found[u] && hv[u].w == -2 && r < nrows) {  // a long row: walk it
                    p[u] = rowptr[r];
                    p1[u] = rowptr[r + 1];
                }
                dg[u] = (hprow && found[u]) ? (int64_t)pdeg[rk[u]] : p1[u] - p[u];
            }
        } else {
            // row bounds are loaded for every row, independently of the mask word
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                const int64_t r = ((w0 + u) << 6) + lane;
                p[u] = p1[u] = 0;
                if (r < nrows) {
                    p[u] = rowptr[r];
                    p1[u] = rowptr[r + 1];
                }
                dg[u] = p1[u] - p[u];
            }
        }
        for (int it = 0; it < p1_steps; it++) {
            bool go[PULL_U], any = false;
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                go[u] = live[u] && !found[u] && p[u] < p1[u];
                any = any || go[u];
            }
            if (!__ballot(any)) break;
            int k[PULL_U][4];
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
#pragma unroll
                for (int t = 0; t < 4; t++) k[u][t] = -1;
                if (go[u]) {
#pragma unroll
                    for (int t = 0; t < 4; t++)
                        if (p[u] + t < p1[u]) k[u][t] = colidx[p[u] + t];
                }
            }
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                if (go[u]) {
                    int f = 0;
                    if (dbg & 32) {  // diagnostics: no frontier probes in the steps
#pragma unroll
                        for (int t = 0; t < 4; t++) f += k[u][t] == 0x7fffffff;
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; t++) f += k[u][t] >= 0 && gb_bit(ubits, k[u][t]);
                    }
                    found[u] = f != 0;
                    p[u] += 4;
                }
            }
        }
        // rows still open -> segment list
        int n = 0;
#pragma unroll
        for (int u = 0; u < PULL_U; u++) {
            const bool pd = live[u] && !found[u] && p[u] < p1[u];
            const unsigned long long bb = __ballot(pd);
            if (pd) {
                const int i = n + __popcll(bb & lt);
                L.p[i] = p[u];
                L.rem[i] = (int32_t)(p1[u] - p[u]);
                L.id[i] = (int16_t)(u * 64 + lane);
            }
            n += __popcll(bb);
        }
        if (lane < PULL_U) L.hitw[lane] = 0;
        if (dbg & 16) n = 0;  // diagnostics: rows left after the steps are dropped
        gb_wlist_walk_pull(L, n, cap0, colidx, ubits);
#pragma unroll
        for (int u = 0; u < PULL_U; u++) {
            if ((L.hitw[u] >> lane) & 1ULL) found[u] = true;
            const unsigned long long word = __ballot(found[u]);
            if (lane == 0 && w0 + u < nwords) {
                tbits[w0 + u] = word;
                cnt += __popcll(word);
            }
        }
        if (hprow) {
            // edges of the next frontier, estimated by the rows' pull-orientation
            // length (already loaded; exact for symmetric matrices): a hint for the
            // next call's push/pull choice only
#pragma unroll
            for (int u = 0; u < PULL_U; u++)
                if (found[u]) mfn += dg[u];
        }
    }
    return cnt;
}

// The pull with its open rows packed (knob iso_pack; needs the pull heads, no lane-per-row
// steps).  The loop above pays its chain of dependent reads (control words, heads, probes, row
// bounds, edges, frontier bits) once per step of 4 words = 256 lane slots, most of them closed
// by the mask or empty.  Here a wave takes its words in groups of PACK_G steps: one lane owns
// one word and one round trip loads the group's control words; the open rows are packed by a
// prefix sum of the words' popcounts into a per-wave LDS list and the chain runs once per batch
// of 256 packed rows.  Found flags go back through LDS words to the lanes that own the output
// words.  Same rows, same probes, same list rounds: results, count, stamp and hint are those of
// the loop above.  Every loop is bounded by counts in registers (groups, batches, list rounds).
#define PACK_G 4                  // steps per group
#define PACK_W (PACK_G * PULL_U)  // words per group, one lane each
struct gb_wpack {
    int16_t ids[PACK_W * 64];           // the group's open rows in order: word in group * 64 + bit
    unsigned long long fw[PACK_W];      // found flags of the packed slots, 64 per word
    unsigned long long rw[PACK_W];      // the group's words of rows_nonempty, by owning lane, and
    uint32_t rk[PACK_W];                // their rank prefixes: a packed row's record is gb_ne_rank of the pair
};
__device__ __forceinline__ long long gb_pull_iso_packed(int64_t nrows, const int64_t *__restrict__ rowptr,
                                                       const int32_t *__restrict__ colidx,
                                                       const uint64_t *__restrict__ ubits,
                                                       const uint64_t *__restrict__ mbits, bool mcomp,
                                                       uint64_t *__restrict__ tbits, gb_wlist &L, gb_wpack &P,
                                                       const int64_t *__restrict__ hprow, long long &mfn, int cap0,
                                                       const uint64_t *__restrict__ rne,
                                                       const uint64_t *__restrict__ qbits, const gb_asg_dev &g,
                                                       long long &adelta, const int32_t *__restrict__ ph,
                                                       const uint32_t *__restrict__ pdeg,
                                                       const uint32_t *__restrict__ nrk) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nwords = (nrows + 63) >> 6;
    const int64_t stride = nwaves * PULL_U;  // words between a wave's steps
    const uint64_t tail = (nrows & 63) ? ((1ULL << (nrows & 63)) - 1) : ~0ULL;
    const unsigned long long lt = (1ULL << lane) - 1;
    long long cnt = 0;
    for (int64_t wb = wave * PULL_U; wb < nwords; wb += stride * PACK_G) {
        // lane l < PACK_W owns word l % PULL_U of the group's step l / PULL_U (as the push's `pre`)
        const int64_t wl = wb + (int64_t)(lane / PULL_U) * stride + (lane & (PULL_U - 1));
        const bool inr = lane < PACK_W && wl < nwords;
        const uint64_t qw = (qbits && inr) ? qbits[wl] : 0;
        const uint64_t mw = (mbits && inr) ? mbits[wl] : 0;
        const uint64_t rw = (rne && inr) ? rne[wl] : ~0ULL;
        const uint32_t nr = inr ? nrk[wl] : 0;  // the heads' rank prefix: the same round trip
        uint64_t mine = ~0ULL;
        if (qbits) {  // fused assign (gb_asg_words): w |= q, w's value at each q bit = x
            if (qw) {
                const uint64_t c = g.bits == mbits ? mw : g.bits[wl], nwd = c | qw;
                if (nwd != c) g.bits[wl] = nwd;
                adelta += (long long)__popcll(nwd) - (long long)__popcll(c);
            }
            for (unsigned long long qb = __ballot(qw != 0); qb; qb &= qb - 1) {
                const int u = __ffsll(qb) - 1;
                const uint64_t word = __shfl(qw, u, 64);
                const int64_t wu = wb + (int64_t)(u / PULL_U) * stride + (u & (PULL_U - 1));
                if ((word >> lane) & 1ULL) gb_store_sized(g.vals, (wu << 6) + lane, g.size, g.x);
            }
            if (mbits) mine = mcomp ? ~(mw | qw) : (mw | qw);
        } else if (mbits) {
            mine = mcomp ? ~mw : mw;
        }
        if (rne) mine &= rw;  // rows without entries produce nothing
        if (wl == nwords - 1) mine &= tail;
        if (!inr) mine = 0;
        // each word's first packed slot: exclusive prefix of the popcounts over the owning lanes
        const int c = __popcll(mine);
        int incl = c;
#pragma unroll
        for (int off = 1; off < PACK_W; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        const int excl = incl - c;
        const int total = __shfl(incl, PACK_W - 1, 64);
        if (!total) {  // nothing open in the group
            if (inr) tbits[wl] = 0;
            continue;
        }
        const unsigned long long ob = __ballot(mine != 0);
        for (unsigned long long b = ob; b; b &= b - 1) {
            const int u = __ffsll(b) - 1;
            const uint64_t word = __shfl(mine, u, 64);
            const int base = __shfl(excl, u, 64);
            if ((word >> lane) & 1ULL) P.ids[base + __popcll(word & lt)] = (int16_t)(u * 64 + lane);
        }
        if (lane < PACK_W) {  // the batch lanes know a row by its owner lane and bit only
            P.rw[lane] = rw;
            P.rk[lane] = nr;
        }
        gb_wave_sync();
        for (int b0 = 0; b0 < total; b0 += 256) {
            bool live[PULL_U], found[PULL_U];
            int64_t r[PULL_U];
            uint32_t rk[PULL_U];
            int4 hv[PULL_U];
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                const int i = b0 + u * 64 + lane;
                live[u] = i < total;
                const int id = live[u] ? P.ids[i] : 0;
                r[u] = ((wb + (int64_t)(id >> 8) * stride + ((id >> 6) & (PULL_U - 1))) << 6) + (id & 63);
                rk[u] = gb_ne_rank(P.rk[id >> 6], P.rw[id >> 6], id & 63);
                hv[u] = make_int4(-1, -1, -1, -1);
                if (live[u]) hv[u] = reinterpret_cast<const int4 *>(ph)[rk[u]];
            }
            gb_pull_probe_heads(hv, ubits, found);
            int64_t p[PULL_U], p1[PULL_U], dg[PULL_U];
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                p[u] = p1[u] = 0;
                if (live[u] && !found[u] && hv[u].w == -2 && r[u] < nrows) {  // a long row: walk it
                    p[u] = rowptr[r[u]];
                    p1[u] = rowptr[r[u] + 1];
                }
                dg[u] = (hprow && found[u]) ? (int64_t)pdeg[rk[u]] : p1[u] - p[u];
            }
            // rows still open -> segment list (ids local to the batch: u * 64 + lane)
            int n = 0;
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                const bool pd = p[u] < p1[u];
                const unsigned long long bb = __ballot(pd);
                if (pd) {
                    const int i = n + __popcll(bb & lt);
                    L.p[i] = p[u];
                    L.rem[i] = (int32_t)(p1[u] - p[u]);
                    L.id[i] = (int16_t)(u * 64 + lane);
                }
                n += __popcll(bb);
            }
            if (lane < PULL_U) L.hitw[lane] = 0;
            gb_wlist_walk_pull(L, n, cap0, colidx, ubits);
#pragma unroll
            for (int u = 0; u < PULL_U; u++) {
                if ((L.hitw[u] >> lane) & 1ULL) found[u] = true;
                const unsigned long long word = __ballot(found[u]);
                if (lane == 0) P.fw[(b0 >> 6) + u] = word;
                if (hprow && found[u]) mfn += dg[u];  // the hint, as in the loop above
            }
            gb_wave_sync();
        }
        // scatter-back: each open row reads its slot's flag; the owning lane stores the word
        unsigned long long res = 0;
        for (unsigned long long b = ob; b; b &= b - 1) {
            const int u = __ffsll(b) - 1;
            const uint64_t word = __shfl(mine, u, 64);
            const int base = __shfl(excl, u, 64);
            bool f = false;
            if ((word >> lane) & 1ULL) {
                const int i = base + __popcll(word & lt);
                f = (P.fw[i >> 6] >> (i & 63)) & 1ULL;
            }
            const unsigned long long fb = __ballot(f);
            if (lane == u) res = fb;
        }
        if (inr) {
            tbits[wl] = res;
            cnt += __popcll(res);
        }
        gb_wave_sync();
    }
    return cnt;
}

// z = mult(a0, u0) for an iso result, types known only at run time (z is x's
// type or bool: the builtin semirings' z types)
template <class X>
__device__ void gb_iso_eval_x(int mul, bool zbool, bool flip, const void *a0, const void *u0, void *out) {
    const X a = a0 ? *(const X *)a0 : X(), b = u0 ? *(const X *)u0 : X();
    const X x = flip ? b : a, y = flip ? a : b;
    if (zbool) *(bool *)out = gb_binop_z<X, bool>(mul, x, y, 0, 0, 0);
    else *(X *)out = gb_binop_z<X, X>(mul, x, y, 0, 0, 0);
}
__device__ void gb_iso_eval(int mul, int xcode, int zcode, bool flip, const void *a0, const void *u0, void *out) {
    const bool zb = zcode == GBAMD_T_BOOL && xcode != GBAMD_T_BOOL;
    switch (xcode) {
    case GBAMD_T_BOOL: gb_iso_eval_x<bool>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_INT8: gb_iso_eval_x<int8_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_UINT8: gb_iso_eval_x<uint8_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_INT16: gb_iso_eval_x<int16_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_UINT16: gb_iso_eval_x<uint16_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_INT32: gb_iso_eval_x<int32_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_UINT32: gb_iso_eval_x<uint32_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_INT64: gb_iso_eval_x<int64_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_UINT64: gb_iso_eval_x<uint64_t>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_FP32: gb_iso_eval_x<float>(mul, zb, flip, a0, u0, out); break;
    case GBAMD_T_FP64: gb_iso_eval_x<double>(mul, zb, flip, a0, u0, out); break;
    default: break;
    }
}

#define GB_ZP_MAX 4  // pooled cleared-vector storages zeroed per iso SpMV launch

struct gb_iso_args {
    // direction: from the frontier's edge-count hint (the vector's producer
    // computed it), else from k_dir_prep's decision, else pull
    const long long *mf_hint;
    gb_dir_rule rule;
    const unsigned long long *dst;
    // next-frontier hint: edges of the output's entries in rows of hprow
    const int64_t *hprow;
    long long *mf_out;
    // iso value of the result: gb_iso_eval(mul, ...) -> iso_out (nullptr: not written)
    int mul, xcode, zcode;
    bool flip;
    const void *a0, *u0;
    void *iso_out;
    // host mailbox for the count; pub_form (knob iso_pub): 0 one tagged word (GB_PUB_TAG) stored
    // relaxed, 1 value + system fence + release seq (round 4), 2 the tagged word stored release
    gb_host_slot *pub;
    long long pub_seq;
    int pub_form;
    // u's exact device count (gb_asg::u_count_exact; nullptr: not known): 0 ends the launch early
    const int64_t *u_exit;
    bool out_zeroed;  // T's bitmap came zeroed (the spare)
    // a bitmap to zero for the next call's push output
    uint64_t *spare;
    int64_t spare_words;
    // pull shape: lane-per-row steps of 4 edges, then the first per-row cap of the list rounds
    int p1_steps, cap0;
    int dbg;                        // diagnostics (knob iso_dbg): 1 no mailbox, 2 no hint sum, 4 no work, 8 empty,
                                    // 16 pull without its segment list, 32 pull steps without probes (wrong results),
                                    // 64 no finish, 128 the round-4 dependent read order (exact; A/B),
                                    // 512 push without the frontier-word prefetch (exact; A/B)
    int pack;                       // open rows packed across a wave's steps (knob iso_pack): 1 pull, 2 push
    bool packed;                    // one-round finish (iso_finish_packed): n < 2^27
    const uint64_t *rows_nonempty;  // pull rows with entries (nullptr: all)
    const uint32_t *ne_rank;        // its per-word exclusive prefix (gb_view_nonempty; the heads' index)
    const int32_t *phead;           // pull head per non-empty row by rank, 4 int32 (nullptr: none; gb_view_pullfirst)
    const uint32_t *pdeg;           // push-orientation length per non-empty pull row (the hint of found rows)
    int host_dir;                   // 1: push, decided on the host (small frontier of known size)
    // storage of cleared vectors zeroed by this launch (gb_zpool_*): bitmaps of zb_words words,
    // counts of 2 + GB_HINT_PARTS words
    uint64_t *zb[GB_ZP_MAX];
    int64_t *zc[GB_ZP_MAX];
    int nzb, nzc;
    int64_t zb_words;
    // fused deferred assign (gb_asg): w<q>(:) = x with q = u (asg.bits nullptr: none)
    gb_asg_dev asg;
    const void *asg_qiso;
    int asg_qiso_code;
    unsigned long long *asg_count;
    int64_t root;  // >= 0: the frontier is this one pending vertex (gb_push_root); u's bits do not hold it
    // diagnostics (environment GRAPHBLAS_AMD_ISO_TS): wall-clock stamps (s_memrealtime, 100 MHz) of
    // each launch's start (block 0) and end (the finishing block), ts[0] / ts[1] launch counters,
    // pairs from ts[2] -- kernel gaps without a profiler (tools/iso_gaps.py)
    unsigned long long *ts;
};

// The result's finish in one round of atomics (n < 2^27): the block sums of the
// count and of the fused assign's count delta travel packed in one 64-bit word
// (arrival 10 bits | count 27 | delta 27) through the sharded grid sum, and the
// next-frontier hint needs no root at all -- each shard's last block stores the
// shard's total in the output's hint parts, which the hint's reader adds up.  All
// of a block's atomics are issued together (one round trip instead of the six of
// three separate grid sums: ~5 us per BFS level).
#define ISO_ARR_BITS 10
#define ISO_VAL_BITS 27

// hand the count to the host without a copy (gb_host_slot_wait)
#define ISO_TS_PAIRS (1 << 20)
__device__ __forceinline__ void iso_ts_mark(const gb_iso_args &a, int which) {
    if (!a.ts) return;
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    const unsigned long long k = atomicAdd(&a.ts[which], 1ULL);
    if (k < ISO_TS_PAIRS) a.ts[2 + 2 * k + which] = t;
}

__device__ __forceinline__ void iso_publish(const gb_iso_args &a, long long tot) {
    iso_ts_mark(a, 1);
    if (!a.pub || (a.dbg & 1)) return;
    if (a.pub_form == 1) {
        __hip_atomic_store(&a.pub->value, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __hip_atomic_store(&a.pub->seq, a.pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const long long w = (long long)(GB_PUB_TAG | (((unsigned long long)a.pub_seq & 0x7fffffffULL) << 32) |
                                    ((unsigned long long)tot & 0xffffffffULL));
    if (a.pub_form == 0) __hip_atomic_store(&a.pub->seq, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else __hip_atomic_store(&a.pub->seq, w, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void iso_finish_packed(long long cnt, long long mfn, long long adelta,
                                                  unsigned long long *__restrict__ tcount,
                                                  unsigned long long *__restrict__ gst, const gb_iso_args &a) {
    __shared__ long long part[3][SPMV_BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        mfn += __shfl_xor(mfn, off, 64);
        adelta += __shfl_xor(adelta, off, 64);
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wid] = cnt;
        part[1][wid] = mfn;
        part[2][wid] = adelta;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    cnt = mfn = adelta = 0;
    for (int w = 0; w < SPMV_BLOCK / 64; w++) {
        cnt += part[0][w];
        mfn += part[1][w];
        adelta += part[2][w];
    }
    const unsigned nb = gridDim.x;
    const unsigned s = blockIdx.x % GB_GRID_SHARDS;
    const unsigned in_shard = (nb - s + GB_GRID_SHARDS - 1) / GB_GRID_SHARDS;
    const unsigned long long AM = (1ULL << ISO_ARR_BITS) - 1, VM = (1ULL << ISO_VAL_BITS) - 1;
    unsigned long long *cs = gst + (size_t)s * GB_GRID_STRIDE;
    unsigned long long *hs = gst + GB_GRID2_OFFSET + (size_t)s * GB_GRID_STRIDE;
    const unsigned long long pk =
        ((unsigned long long)adelta << (ISO_ARR_BITS + ISO_VAL_BITS)) | ((unsigned long long)cnt << ISO_ARR_BITS) | 1ULL;
    unsigned long long oh = 0;
    if (a.mf_out) {
        oh = atomicAdd(hs, ((unsigned long long)mfn << 12) + 1ULL);
        if (blockIdx.x == 0)  // the parts of shards no block maps to
            for (unsigned i = nb; i < GB_HINT_PARTS; i++) a.mf_out[i] = 0;
    }
    const unsigned long long oc = atomicAdd(cs, pk);
    if (a.mf_out && (unsigned)(oh & 0xFFF) + 1 == in_shard) {
        a.mf_out[s] = (long long)(oh >> 12) + mfn;  // this shard's part of the hint
        atomicExch(hs, 0ULL);
    }
    if ((unsigned)(oc & AM) + 1 != in_shard) return;
    atomicExch(cs, 0ULL);
    const unsigned long long scnt = ((oc >> ISO_ARR_BITS) & VM) + (unsigned long long)cnt;
    const unsigned long long sadd = (oc >> (ISO_ARR_BITS + ISO_VAL_BITS)) + (unsigned long long)adelta;
    const unsigned nshards = nb < GB_GRID_SHARDS ? nb : GB_GRID_SHARDS;
    unsigned long long *root = gst + (size_t)GB_GRID_SHARDS * GB_GRID_STRIDE;
    const unsigned long long o2 =
        atomicAdd(root, (sadd << (ISO_ARR_BITS + ISO_VAL_BITS)) | (scnt << ISO_ARR_BITS) | 1ULL);
    if ((unsigned)(o2 & AM) + 1 != nshards) return;
    const long long tot = (long long)(((o2 >> ISO_ARR_BITS) & VM) + scnt);
    const long long add = (long long)((o2 >> (ISO_ARR_BITS + ISO_VAL_BITS)) + sadd);
    *tcount = (unsigned long long)tot;
    iso_publish(a, tot);
    // after the publish (off the host's critical path; the next launch on the stream starts
    // only after this kernel has ended): the root reset and the fused assign's count
    atomicExch(root, 0ULL);
    if (a.asg.bits && add) atomicAdd(a.asg_count, (unsigned long long)add);
}

// One launch does the chosen direction and finishes the result: count
// (stored, no prior zeroing needed), next-frontier hint, iso value, mailbox.
__global__ __launch_bounds__(SPMV_BLOCK) void k_iso_work(
    int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
    int64_t nwords_u, const uint64_t *__restrict__ ubits, const int64_t *__restrict__ prow,
    const int32_t *__restrict__ pcol, const int32_t *__restrict__ hubs, int64_t nhubs, int64_t H,
    const uint64_t *__restrict__ mbits, bool mcomp, uint64_t *__restrict__ tbits,
    unsigned long long *__restrict__ tcount, unsigned long long *__restrict__ gst, gb_iso_args a) {
    __shared__ gb_wlist lists[WAVES_PER_BLOCK];
    gb_wlist &L = lists[threadIdx.x >> 6];
    __shared__ gb_wpack packs[WAVES_PER_BLOCK];
    if (a.ts && blockIdx.x == 0 && threadIdx.x == 0) iso_ts_mark(a, 0);
    if (a.dbg & 8) return;  // diagnostics: the launch alone
    bool push = false;
    if (a.host_dir == 1) {
        push = true;
    } else if (a.mf_hint) {
        long long mf = 0;  // the hint's parts (one per grid-sum shard of its producer)
        for (int i = 0; i < GB_HINT_PARTS; i++) mf += a.mf_hint[i];
        push = gb_dir_decide(mf, a.rule);
    }
    else if (a.dst) push = a.dst[ST_PUSH] != 0;
    if (a.spare && !(a.dbg & 32)) {  // dbg 32: diagnostics, no zeroing
        for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < a.spare_words;
             w += (int64_t)gridDim.x * blockDim.x)
            a.spare[w] = 0;
    }
    for (int j = 0; j < ((a.dbg & 32) ? 0 : a.nzb); j++)  // cleared vectors' bitmaps, back to the pool zeroed
        for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < a.zb_words;
             w += (int64_t)gridDim.x * blockDim.x)
            a.zb[j][w] = 0;
    if (blockIdx.x == 0)
        for (int j = 0; j < a.nzc; j++)
            for (int w = threadIdx.x; w < 2 + GB_HINT_PARTS; w += blockDim.x) a.zc[j][w] = 0;
    // the result's iso value does not depend on the work: evaluated here, off the finish's path
    if (a.packed && a.iso_out && blockIdx.x == 0 && threadIdx.x == 0)
        gb_iso_eval(a.mul, a.xcode, a.zcode, a.flip, a.a0, a.u0, a.iso_out);
    if (a.u_exit && *a.u_exit == 0) {
        // an empty u (the speculated level after a BFS's last): no products, an empty stamp, so
        // no grid-wide finish -- block 0 stores the zero count and hint and publishes
        if (!a.out_zeroed)
            for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < ((nrows + 63) >> 6);
                 w += (int64_t)gridDim.x * blockDim.x)
                tbits[w] = 0;
        if (blockIdx.x == 0) {
            if (a.mf_out)
                for (int i = threadIdx.x; i < GB_HINT_PARTS; i += blockDim.x) a.mf_out[i] = 0;
            if (threadIdx.x == 0) {
                *tcount = 0ULL;
                if (!a.packed && a.iso_out) gb_iso_eval(a.mul, a.xcode, a.zcode, a.flip, a.a0, a.u0, a.iso_out);
                iso_publish(a, 0);
            }
        }
        return;
    }
    // fused assign: q's value mask is empty when q is iso with a false value
    const uint64_t *qbits = nullptr;
    if (a.asg.bits && (!a.asg_qiso || gb_dyn_nonzero(a.asg_qiso, a.asg_qiso_code))) qbits = ubits;
    long long mfn = 0, cnt = 0, adelta = 0;
    if ((a.root >= 0 || push) && blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd(gst + GB_DIR_STATE_OFFSET + ST_PUSHES, 1ULL);  // result unused: nothing waits for it
    // push: the hint's row lengths (the hub table's section; hprow is the push orientation's
    // row pointers)
    const uint32_t *hlen = (a.hprow && hubs) ? gb_hub_sections_of(hubs, nhubs).rowlen : nullptr;
    if (a.dbg & 4)
        ;
    else if (a.root >= 0)
        cnt = gb_push_root(a.root, prow, pcol, mbits, mcomp, (unsigned long long *)tbits, hlen, mfn,
                           a.asg.bits != nullptr, a.asg, adelta);
    else if (push)
        cnt = gb_push_phase(nwords_u, ubits, prow, pcol, hubs, nhubs, H, mbits, mcomp,
                            (unsigned long long *)tbits, L, hlen, mfn, qbits, a.asg, adelta,
                            (a.dbg & 128) != 0, (a.dbg & 512) == 0, (a.pack & 2) != 0);
    else {
        // the heads are found through the non-empty bitmap's ranks: without it, no heads
        const int32_t *ph =
            (a.phead && a.rows_nonempty && a.ne_rank && (!a.hprow || a.pdeg)) ? a.phead : nullptr;
        if ((a.pack & 1) && ph && a.p1_steps == 0 && !(a.dbg & (16 | 32 | 128)))
            cnt = gb_pull_iso_packed(nrows, rowptr, colidx, ubits, mbits, mcomp, tbits, L, packs[threadIdx.x >> 6],
                                     a.hprow, mfn, a.cap0, a.rows_nonempty, qbits, a.asg, adelta, ph, a.pdeg, a.ne_rank);
        else
            cnt = gb_pull_iso_phase(nrows, rowptr, colidx, ubits, mbits, mcomp, tbits, L, a.hprow, mfn, a.p1_steps,
                                    a.cap0, a.rows_nonempty, qbits, a.asg, adelta, a.dbg, ph, a.pdeg, a.ne_rank);
    }
    if (a.dbg & 64) return;  // diagnostics: no finish (count, hint, mailbox)
    if (a.packed) {
        iso_finish_packed(cnt, mfn, adelta, tcount, gst, a);
        return;
    }
    long long tot;
    if (gb_grid_sum(cnt, gst, &tot)) {
        *tcount = (unsigned long long)tot;
        if (a.iso_out) gb_iso_eval(a.mul, a.xcode, a.zcode, a.flip, a.a0, a.u0, a.iso_out);
        iso_publish(a, tot);
    }
    if (a.mf_out && !(a.dbg & 2)) {
        long long m;
        if (gb_grid_sum(mfn, gst + GB_GRID2_OFFSET, &m)) {
            a.mf_out[0] = m;
            for (int i = 1; i < GB_HINT_PARTS; i++) a.mf_out[i] = 0;
        }
    }
    if (a.asg.bits) gb_grid_add(adelta, a.asg_count, gst + GB_GRID3_OFFSET);
}

// ---------------------------------------------------------------- host side
static std::mutex g_dir_mu;  // keeps the prep/push/pull launches of one call adjacent
static unsigned long long *g_iso_ts = nullptr;  // GRAPHBLAS_AMD_ISO_TS diagnostics buffer
static unsigned long long *iso_ts_buffer() {
    static const bool on = getenv("GRAPHBLAS_AMD_ISO_TS") != nullptr;
    if (!on) return nullptr;
    if (!g_iso_ts) {
        GB_HIP(hipMalloc((void **)&g_iso_ts, (2 + 2 * (size_t)ISO_TS_PAIRS) * sizeof(unsigned long long)));
        GB_HIP(hipMemset(g_iso_ts, 0, (2 + 2 * (size_t)ISO_TS_PAIRS) * sizeof(unsigned long long)));
        GB_HIP(hipDeviceSynchronize());
    }
    return g_iso_ts;
}
// writes the stamps to the file GRAPHBLAS_AMD_ISO_TS names (raw u64: starts, ends, pairs); returns the
// launch count (GxB_Global_get_int("iso_ts_dump"))
int64_t gb_iso_ts_dump() {
    const char *path = getenv("GRAPHBLAS_AMD_ISO_TS");
    if (!path || !g_iso_ts) return 0;
    GB_HIP(hipStreamSynchronize(gb_stream()));
    unsigned long long c[2];
    GB_HIP(hipMemcpy(c, g_iso_ts, sizeof(c), hipMemcpyDeviceToHost));
    const size_t k = std::min<unsigned long long>(std::min(c[0], c[1]), ISO_TS_PAIRS);
    std::vector<unsigned long long> buf(2 + 2 * k);
    GB_HIP(hipMemcpy(buf.data(), g_iso_ts, buf.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    fwrite(buf.data(), sizeof(unsigned long long), buf.size(), f);
    fclose(f);
    return (int64_t)k;
}
static uint64_t *g_spare = nullptr;  // zeroed bitmap for the next iso SpMV's output (under g_dir_mu)
static int64_t g_spare_words = 0;

// ---- pool of zeroed vector storage (under g_dir_mu): bitmaps of one size (g_zp_words) and
// counts; `dirty` ones are zeroed by the next k_iso_work launch, then become `ready`
static std::vector<uint64_t *> g_zp_ready_b, g_zp_dirty_b;
static std::vector<int64_t *> g_zp_ready_c, g_zp_dirty_c;
static int64_t g_zp_words = 0;

bool gb_zpool_clear_vector(GB_Obj *v) {
    if (gb_knob("zero_pool") == 1) return false;
    std::lock_guard<std::mutex> lk(g_dir_mu);
    const int64_t nw = gb_words(v->nrows);
    if (nw != g_zp_words) {  // a new size: the pool follows the most recent one
        for (auto *p : g_zp_ready_b) gb_free(p);
        for (auto *p : g_zp_dirty_b) gb_free(p);
        g_zp_ready_b.clear();
        g_zp_dirty_b.clear();
        g_zp_words = nw;
    }
    if (v->bits && (int)g_zp_dirty_b.size() < GB_ZP_MAX) {  // the old bitmap, to be zeroed later
        g_zp_dirty_b.push_back(v->bits);
        v->bits = nullptr;
    }
    if (g_zp_ready_b.empty() || g_zp_ready_c.empty()) return false;
    gb_cw_release(v);
    gb_free(v->bits);
    gb_free(v->dense);
    gb_free(v->d_nvals);
    v->bits = g_zp_ready_b.back();
    g_zp_ready_b.pop_back();
    v->d_nvals = g_zp_ready_c.back();
    g_zp_ready_c.pop_back();
    v->dense = nullptr;
    v->iso = false;
    v->nvals = 0;
    v->nvals_valid = true;
    v->hint_valid = false;
    v->pub_seq = 0;
    return true;
}

// blocks of k_iso_work the device holds at once (the work grid is sized to one wave of blocks)
static int64_t iso_work_resident_blocks() {
    static int64_t cap = 0;
    if (!cap) {
        int dev = 0, cus = 0, per = 0;
        GB_HIP(hipGetDevice(&dev));
        GB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        GB_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_iso_work, SPMV_BLOCK, 0));
        cap = std::max<int64_t>(1, (int64_t)cus * std::max(per, 1));
    }
    return cap;
}

// The iso-result SpMV behind gb_spmv: T is allocated (bitmap, one value, count words), n > 0;
// av / uv are the operands' values as the multiplier's input type (nullptr: not read).
void gb_spmv_iso(gb_vec_result &T, const gb_csr_view &A, const gb_csr_view *Apush, gb_bitmap_view &u,
                 const gb_vmask &mask, GrB_Semiring sr, bool flip, const gb_asg *asg, const void *av,
                 const void *uv) {
    const gb_sr_info info = gb_sr_describe(sr);
    // gb_iso_eval writes z as x's type or bool: the builtin multipliers' z types
    GB_REQUIRE(info.zcode == info.xcode || info.zcode == GBAMD_T_BOOL, GrB_NOT_IMPLEMENTED,
               "semiring type combination not supported");
    const int64_t n = A.nrows;
    const int64_t dir_knob = gb_knob("spmv_direction");  // 0 auto, 1 pull only, 2 push only
    const bool can_push = Apush && Apush->nrows == u.n && Apush->hubs && dir_knob != 1;
    int64_t alpha = gb_knob("push_alpha");
    // Beamer's alpha, swept with tools/ab_bfs.py (s22, 16 roots, 8 interleaved rounds; two boxes):
    // 14 -> 0.312 / 0.328 ms per BFS, 36 -> 0.299 / 0.318, 48 -> 0.2985, 64 -> 0.314, 96 -> 0.323
    if (alpha <= 0) alpha = 48;
    const int64_t nw = gb_words(n);
    unsigned long long *gst = gb_device_state();
    unsigned long long *dst = gst + GB_DIR_STATE_OFFSET;
    const int64_t uw = gb_words(u.n);
    int64_t units = (nw + PULL_U - 1) / PULL_U;  // waves the pull wants
    std::lock_guard<std::mutex> lk(g_dir_mu);  // the spare bitmap and the direction state
    gb_iso_args args{};
    args.rule = gb_dir_rule{mask.count, asg ? u.count : nullptr, mask.comp, n, A.nvals, alpha, dir_knob == 2};
    if (asg) {
        GB_REQUIRE(u.n == n, GrB_INVALID_VALUE, "fused assign needs u and w of one size");
        args.asg = gb_asg_dev{asg->bits, asg->vals, asg->size, asg->x};
        args.asg_qiso = asg->q_iso;
        args.asg_qiso_code = asg->q_iso_code;
        args.asg_count = (unsigned long long *)asg->count;
    }
    args.dbg = (int)gb_knob("iso_dbg");
    // open rows packed across a wave's steps: 0 pull and push (default), 1 neither (the
    // per-step loops), 2 pull only, 3 push only
    const int64_t pack_knob = gb_knob("iso_pack");
    args.pack = ((pack_knob == 0 || pack_knob == 2) ? 1 : 0) | ((pack_knob == 0 || pack_knob == 3) ? 2 : 0);
    args.ts = iso_ts_buffer();
    args.root = asg ? asg->root : -1;
    GB_REQUIRE(args.root < 0 || can_push, GrB_PANIC, "a pending root needs the push orientation");
    args.packed = n < (1LL << ISO_VAL_BITS) && u.n < (1LL << ISO_VAL_BITS) && gb_knob("iso_packed") != 1;
    if (args.dbg & 1) T.pub = nullptr;  // diagnostics: the host reads the count by a copy
    // lane-per-row steps after the pull heads: none by default (tools/gpu_ab2.sh, s22
    // any_pair: 0.340 ms/BFS without, 0.356 with 2, 0.350 with 1)
    args.p1_steps = (int)gb_knob("pull_steps");
    if (args.p1_steps < 0) args.p1_steps = 0;
    // first per-row cap of the pull's segment-list rounds: tools/ab_bfs.py (s22, 6 interleaved
    // rounds, after the two-round head probes): 16 -> 0.2285, 32 -> 0.2266, 64 -> 0.2260 ms/BFS
    args.cap0 = (int)gb_knob("pull_cap");
    if (args.cap0 <= 0) args.cap0 = 64;
    args.rows_nonempty = A.nonempty;
    args.ne_rank = A.ne_rank;
    args.phead = A.phead;
    args.pdeg = A.pdeg;
    // the result's iso value: evaluated by k_iso_work (gb_iso_eval), its only writer
    args.mul = info.mul;
    args.xcode = info.xcode;
    args.zcode = info.zcode;
    args.flip = flip;
    args.a0 = av;
    args.u0 = uv;
    args.iso_out = T.dense;
    args.pub = T.pub ? gb_host_slot_device(T.pub) : nullptr;
    args.pub_seq = (long long)T.pub_seq;
    // the count travels in one tagged word stored without a fence: the host needs only the
    // count, and the kernel's end orders everything else for the next launch.  With the
    // BFS speculation on, tools/ab_bfs.py (s22, 8 interleaved rounds): 0.2298 ms per BFS
    // vs 0.2325 with value + system fence + release seq (round 3 had measured the reverse
    // without speculation, when the host waited on every mailbox)
    args.pub_form = n < (1LL << 31) ? (int)std::max<int64_t>(0, std::min<int64_t>(2, gb_knob("iso_pub"))) : 1;
    // a zeroed output bitmap left by the previous call (push may write into it directly)
    bool spare_taken = false;
    if (g_spare && g_spare_words == nw) {
        gb_free(T.bits);
        T.bits = g_spare;
        spare_taken = true;
    } else if (g_spare) {
        gb_free(g_spare);
    }
    g_spare = nullptr;
    g_spare_words = 0;
    args.out_zeroed = spare_taken;
    if (asg && asg->u_count_exact && u.count && asg->root < 0 && gb_knob("spec_empty_exit") != 1)
        args.u_exit = u.count;
    bool need_prep = false;
    if (can_push) {
        units = std::max<int64_t>(units, std::max<int64_t>((Apush->nhubs + 15) / 16, (uw + 3) / 4));
        if (n == u.n) {  // outputs index the same vertex space as u: they can seed the next call
            args.hprow = Apush->rowptr;
            args.mf_out = (long long *)(T.d_nvals + 2);
            T.hint_key = Apush->rowptr;
        }
        const bool hint_ok = u.mf_hint && u.hint_key == Apush->rowptr;
        // no hint (a frontier set by the host, e.g. a BFS root): push is certain when even
        // every frontier vertex having the longest row stays under the pull's least work
        bool push_sure = false;
        if (!hint_ok && spare_taken && u.h_nvals >= 0 && Apush->maxdeg >= 0 &&
            gb_knob("host_dir") != 1) {
            // open rows (where the output may be written) from below.  mask.h_count is the
            // mask's set-bit count; do_spmv fills it from a stored-entry count (an upper
            // bound on the set bits of a value mask, whose stored entries may be false)
            // only for structural or complemented masks, or when the mask is empty -- so
            // for a plain value mask it is never an over-estimate (tests/test_gpu_parity.py::
            // test_value_mask_false_entries_no_host_push)
            int64_t open_lo = -1;
            if (!mask.bits) {
                open_lo = n;
            } else if (mask.h_count >= 0) {
                const int64_t mc_hi = std::min<int64_t>(n, mask.h_count + (asg ? u.h_nvals : 0));
                open_lo = mask.comp ? n - mc_hi : mask.h_count;
            }
            const double avg = n ? (double)A.nvals / (double)n : 0.0;
            push_sure = open_lo >= 0 &&
                        (double)u.h_nvals * (double)Apush->maxdeg * (double)alpha < (double)open_lo * avg;
        }
        if (args.root >= 0) {
            // the frontier is one vertex the host knows; the push writes T's bitmap directly, so
            // it must start zeroed (the spare usually is; a first call zeroes it here)
            if (!spare_taken) gb_memset(T.bits, 0, nw * sizeof(uint64_t));
            args.out_zeroed = true;
            args.host_dir = 1;
            g_stat_host_push.fetch_add(1, std::memory_order_relaxed);
            gb_stat_add("bfs_root_push", 1);
        } else if (hint_ok && spare_taken) {
            args.mf_hint = u.mf_hint;  // decide in the work kernel: one launch
        } else if (push_sure) {
            args.host_dir = 1;  // one launch, no prep
            g_stat_host_push.fetch_add(1, std::memory_order_relaxed);
        } else {
            need_prep = true;
        }
    }
    if (need_prep) {
        // prep (frontier edges -> direction, zeroed output), then the work launch
        int64_t pcap = gb_knob("prep_grid");
        if (pcap <= 0) pcap = 1024;
        const unsigned prep_grid =
            (unsigned)std::max<int64_t>(1, std::min<int64_t>((uw + 63) / 64, pcap));
        hipLaunchKernelGGL(k_dir_prep, dim3(prep_grid), dim3(SPMV_BLOCK), 0, gb_stream(), u.bits, uw,
                           Apush->rowptr, gst, dst, T.bits, nw, (unsigned long long *)T.d_nvals, args.rule);
        GB_LAUNCH_CHECK();
        args.mf_hint = nullptr;
        args.dst = dst;
    }
    if (can_push) {  // zeroed by this launch, for the next call's push output
        args.spare = gb_malloc_n<uint64_t>(nw);
        args.spare_words = nw;
    }
    // cleared vectors' storage (gb_zpool_clear_vector): zeroed by this launch, then ready
    while ((int)(g_zp_ready_c.size() + g_zp_dirty_c.size()) < GB_ZP_MAX)
        g_zp_dirty_c.push_back(gb_malloc_n<int64_t>(2 + GB_HINT_PARTS));
    args.nzb = (int)std::min<size_t>(g_zp_dirty_b.size(), GB_ZP_MAX);
    for (int j = 0; j < args.nzb; j++) args.zb[j] = g_zp_dirty_b[j];
    args.zb_words = g_zp_words;
    args.nzc = (int)std::min<size_t>(g_zp_dirty_c.size(), GB_ZP_MAX);
    for (int j = 0; j < args.nzc; j++) args.zc[j] = g_zp_dirty_c[j];
    if (args.dbg & (8 | 32)) {
        // diagnostics that return before (8) or skip (32) the zeroing: nothing handed to this
        // launch may be treated as zeroed afterwards
        args.nzb = args.nzc = 0;
        if (args.spare) gb_free(args.spare);
        args.spare = nullptr;
        args.spare_words = 0;
    }
    int64_t gcap = gb_knob("iso_work_grid");
    if (gcap <= 0) gcap = iso_work_resident_blocks();
    // a frontier the host knows to be tiny (the BFS loop reads nvals every level): a small
    // grid -- the work is a few rows, and the finish's grid-wide sum and the drain of
    // fewer blocks are what the level costs
    const int64_t small_n = gb_knob("iso_small_n");
    if (small_n > 0 && u.h_nvals >= 0 && u.h_nvals <= small_n) {
        int64_t sg = gb_knob("iso_small_grid");
        if (sg <= 0) sg = 64;
        gcap = std::min<int64_t>(gcap, sg);
    }
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 3) / 4, gcap));
    if (grid >= GB_GRID_SHARDS * ((1u << ISO_ARR_BITS) - 1)) args.packed = false;  // arrival field
    GB_HPROF(5, "k_iso_work launch");
    hipLaunchKernelGGL(k_iso_work, dim3(grid), dim3(SPMV_BLOCK), 0, gb_stream(), n, A.rowptr, A.colidx, uw,
                       u.bits, can_push ? Apush->rowptr : nullptr, can_push ? Apush->colidx : nullptr,
                       can_push ? Apush->hubs : nullptr, can_push ? Apush->nhubs : 0,
                       can_push ? Apush->hub_H : 1, mask.bits, mask.comp, T.bits,
                       (unsigned long long *)T.d_nvals, gst, args);
    GB_LAUNCH_CHECK();
    g_spare = args.spare;
    g_spare_words = args.spare ? nw : 0;
    for (int j = 0; j < args.nzb; j++) g_zp_ready_b.push_back(args.zb[j]);
    g_zp_dirty_b.erase(g_zp_dirty_b.begin(), g_zp_dirty_b.begin() + args.nzb);
    for (int j = 0; j < args.nzc; j++) g_zp_ready_c.push_back(args.zc[j]);
    g_zp_dirty_c.erase(g_zp_dirty_c.begin(), g_zp_dirty_c.begin() + args.nzc);
    T.published = T.pub != nullptr;
}
