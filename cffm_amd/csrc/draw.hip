// Ranked lists drawn BY LIST ID (cffm_draw_lists, include/cffm_hip.h): list g of a call has the id list0 + g and
// is a function of (seed, id) alone - its positive at[g] among U distinct tuples, m distinct others, the positive at a drawn place -
// so an epoch's lists are the same lists under every split into calls.  cffm_amd/spec.py draw_lists() is the numpy twin and the
// specification; everything here is integer arithmetic and matches it exactly.
//
//   words      word i of a list = output word i & 3 of Philox4x32-10, key = (seed lo, seed hi), counter = (id lo, id hi, i >> 2, 2)
//              (the table draw holds 0 and 1 in that last counter word); m + 1 words, whatever the data
//   negatives  the length-m prefix of a Fisher-Yates shuffle of 0 .. U - 2: step i swaps position i with
//              t = i + ((w_i * (U - 1 - i)) >> 32).  The permutation is carried as a sparse map position -> value (absent =
//              identity) of at most m entries; a value >= at[g] moves up by one (the set without the target)
//   place      (w_m * (m + 1)) >> 32; the negatives keep their order around it
//
// One wavefront per list, four lists per workgroup, and NO workgroup barrier: a wavefront past the last list returns at once, the
// others never wait for it (DESIGN.md 3.1 stage 3).  A wavefront's three arrays (words, map keys, map values; m + 1 words each,
// rounded up to four) live in its own slice of the dynamic LDS.  Lanes draw the words in parallel, one Philox call per four words.
// The chain of m steps is serial: a lookup compares 64 map keys per pass across the lanes and takes the ballot, so the trip counts
// and the branches are wave-uniform; lane 0 writes the step's result.  Same-wavefront LDS traffic is ordered by wavefront-scope
// fences (the hardware runs a wavefront's LDS instructions in order; the fence keeps the compiler from moving them).  The final
// indices go back to LDS so that the gather of the cand rows and the stores run coalesced over (p, a).
#include "internal.hpp"
#include "philox.hpp"

#define DL_WAVES 4        // lists per workgroup
#define DL_TAG 2u         // the list draw's value of the fourth counter word

__device__ __forceinline__ void dl_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64 * DL_WAVES) void draw_lists_kernel(uint32_t k0, uint32_t k1, uint64_t list0, int G,
                                                                   const int32_t* __restrict__ at, uint32_t U, int m, int W,
                                                                   const int32_t* __restrict__ cand, int nf,
                                                                   int32_t* __restrict__ lists_out, int32_t* __restrict__ tuples_out,
                                                                   int32_t* __restrict__ target_out) {
    extern __shared__ uint32_t dl_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * DL_WAVES + wave;
    if (g >= G) return;                                  // wave-uniform; nothing below waits for another wavefront
    uint32_t* wrd = dl_lds + (size_t)wave * 3 * W;       // the words; word i becomes the value chosen at step i
    uint32_t* key = wrd + W;                             // map keys, then the list's final indices
    uint32_t* val = key + W;
    const int Lg = m + 1;
    const int64_t o = (int64_t)g * Lg;
    const int32_t a = at[g];
    if (a < 0 || (uint32_t)a >= U) {                     // defined: no target, an index row of -1, a tuple row of zeros
        if (lists_out)
            for (int p = lane; p < Lg; p += 64) lists_out[o + p] = -1;
        if (tuples_out)
            for (int e = lane; e < Lg * nf; e += 64) tuples_out[o * nf + e] = 0;
        if (lane == 0) target_out[g] = -1;
        return;
    }
    const uint64_t id = list0 + (uint64_t)g;
    for (int q = lane; 4 * q < Lg; q += 64) {            // 4 q + 3 < W: W is Lg rounded up to four
        uint32_t x[4];
        philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), (uint32_t)q, DL_TAG, k0, k1, x);
        wrd[4 * q] = x[0]; wrd[4 * q + 1] = x[1]; wrd[4 * q + 2] = x[2]; wrd[4 * q + 3] = x[3];
    }
    dl_wave_fence();
    const uint32_t n = U - 1u;
    int cnt = 0;                                         // map entries, <= i at step i
    for (int i = 0; i < m; ++i) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(wrd[i]);
        const uint32_t t = (uint32_t)i + __umulhi(w, n - (uint32_t)i);             // i <= t < n <= 2^31 - 2
        int pt = -1, pi = -1;
        for (int s = 0; s < cnt; s += 64) {
            const int idx = s + lane;
            const uint32_t k = idx < cnt ? key[idx] : 0xffffffffu;                 // no key is that large
            const unsigned long long bt = __ballot(k == t), bi = __ballot(k == (uint32_t)i);
            if (bt) pt = s + __ffsll(bt) - 1;                                      // a key sits in the map once
            if (bi) pi = s + __ffsll(bi) - 1;
        }
        const uint32_t vt = pt >= 0 ? __builtin_amdgcn_readfirstlane(val[pt]) : t;
        const uint32_t vi = pi >= 0 ? __builtin_amdgcn_readfirstlane(val[pi]) : (uint32_t)i;
        dl_wave_fence();
        if (lane == 0) {
            const int slot = pt >= 0 ? pt : cnt;                                   // map[t] = vi: t's entry, or a new one; slot <= i < m
            wrd[i] = vt;
            key[slot] = t;
            val[slot] = vi;
        }
        cnt += pt < 0 ? 1 : 0;
        dl_wave_fence();
    }
    const int place = (int)__umulhi(__builtin_amdgcn_readfirstlane(wrd[m]), (uint32_t)Lg);
    for (int p = lane; p < Lg; p += 64) {
        uint32_t v = (uint32_t)a;
        if (p != place) {
            const uint32_t c = wrd[p - (p > place ? 1 : 0)];                       // a word index in [0, m)
            v = c + (c >= (uint32_t)a ? 1u : 0u);
        }
        key[p] = v;
        if (lists_out) lists_out[o + p] = (int32_t)v;
    }
    if (lane == 0) target_out[g] = place;
    if (tuples_out) {
        dl_wave_fence();
        for (int e = lane; e < Lg * nf; e += 64) {
            const int p = e / nf, c = e - p * nf;
            tuples_out[o * nf + e] = cand[(int64_t)key[p] * nf + c];              // key[p] < U
        }
    }
}

// What both entry points refuse, given a U their own check let through (U >= 1, so U - 1 does not wrap).
static bool draw_args_ok(int64_t list0, int32_t G, const int32_t* at, int32_t U, int32_t m, const int32_t* cand, int32_t nf,
                         const int32_t* lists_out, const int32_t* tuples_out, const int32_t* target_out) {
    if (m < 1 || m > U - 1 || m > 1023 || G < 0 || list0 < 0 || list0 > INT64_MAX - (int64_t)G || nf < 0) return false;
    const int64_t slots = (int64_t)G * (m + 1);                                    // < 2^41
    if (slots >= (1ll << 31) || slots * (nf > 1 ? nf : 1) >= (1ll << 31)) return false;
    if ((cand == nullptr) != (tuples_out == nullptr)) return false;
    if (nf == 0 && cand) return false;
    if (!lists_out && !tuples_out) return false;
    return at && target_out;
}

extern "C" int cffm_draw_lists(uint64_t seed, int64_t list0, int32_t G, const int32_t* at, int32_t U, int32_t m, const int32_t* cand,
                               int32_t nf, int32_t* lists_out, int32_t* tuples_out, int32_t* target_out, void* stream) {
    if (U < 2 || !draw_args_ok(list0, G, at, U, m, cand, nf, lists_out, tuples_out, target_out)) return CFFM_ERR_BAD_SHAPE;
    if (G == 0) return 0;
    const int W = (m + 1 + 3) & ~3;
    const size_t lds = (size_t)DL_WAVES * 3 * W * sizeof(uint32_t);                // at most 48 KiB
    const int nb = (G + DL_WAVES - 1) / DL_WAVES;
    hipLaunchKernelGGL(draw_lists_kernel, dim3(nb), dim3(64 * DL_WAVES), lds, (hipStream_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint64_t)list0, G, at, (uint32_t)U, m, W, cand, nf, lists_out, tuples_out, target_out);
    CFFM_CHECK_LAUNCH();
    return 0;
}

// ---- weighted lists (cffm_draw_lists_weighted): the negatives in proportion to weights, by rejection ------------
// cffm_amd/spec.py draw_lists_weighted() is the numpy twin and the specification; integer arithmetic, matched exactly.
//
//   words       word i of a list = output word i & 3 of Philox4x32-10 at counter (id lo, id hi, i >> 2, 3); the place word is output
//               word 0 at counter (id lo, id hi, 0xffffffff, 3)
//   candidate   r = (w * T) >> 32 with T = cdf[U - 1]; j = #{cdf <= r}, a binary search that stays inside [0, U - 1]
//   acceptance  sequential in word order: j is accepted iff it is not at[g] and was not accepted before; the negatives are the first
//               m accepted.  At most 64 * (8 * ceil((m + 1) / 64) + 8) words; a list still short of m then is incomplete and gets
//               the row of a list without a target (-1 / zeros / target -1), as does T == 0
//
// The layout of draw_lists_kernel: one wavefront per list, four per workgroup, no workgroup barrier, the wavefront's two arrays
// (the accepted indices, the final list; W words each) in its own slice of the dynamic LDS, wavefront-scope fences.  Words go in
// rounds of 64, one per lane.  A lane draws its word (the four lanes of a block each make the block's call), searches the cdf
// (bits(U - 1) dependent loads, the lanes in parallel, every lane the same trip count), and tests its candidate against the target
// and against the accepted set, which every lane reads four entries at a time at the same address (unused entries hold 0xffffffff,
// which no index equals).  Among the lanes that pass, a candidate held by an earlier lane of the round loses to it: the loop walks
// the ballot of the passing lanes and broadcasts each one's candidate.  What remains is, in lane order, exactly what the sequential
// rule accepts; a ballot and a prefix count hand out the slots and slots past m - 1 are dropped (the round is truncated where the
// m-th acceptance falls).  Every trip count and branch is wave-uniform; the round cap bounds the time.
#define DLW_TAG 3u
#define DLW_PLACE 0xffffffffu

__global__ __launch_bounds__(64 * DL_WAVES) void draw_lists_weighted_kernel(uint32_t k0, uint32_t k1, uint64_t list0, int G,
                                                                            const int32_t* __restrict__ at, uint32_t U, int m, int W,
                                                                            int steps, int rounds, const uint32_t* __restrict__ cdf,
                                                                            const int32_t* __restrict__ cand, int nf,
                                                                            int32_t* __restrict__ lists_out,
                                                                            int32_t* __restrict__ tuples_out,
                                                                            int32_t* __restrict__ target_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dlw_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * DL_WAVES + wave;
    if (g >= G) return;                                  // wave-uniform; nothing below waits for another wavefront
    uint32_t* acc = dlw_lds + (size_t)wave * 2 * W;       // the accepted indices in acceptance order; W % 4 == 0, 16-byte aligned
    uint32_t* key = acc + W;                             // the list's final indices
    const int Lg = m + 1;
    const int64_t o = (int64_t)g * Lg;
    const int32_t a = at[g];
    const uint32_t T = cdf[U - 1u];
    const uint64_t id = list0 + (uint64_t)g;
    int cnt = 0;                                         // accepted so far, wave-uniform
    if (a >= 0 && (uint32_t)a < U && T != 0u) {
        for (int p = lane; p < W; p += 64) acc[p] = 0xffffffffu;
        dl_wave_fence();
        for (int r = 0; r < rounds && cnt < m; ++r) {
            uint32_t x[4];
            philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), (uint32_t)(16 * r + (lane >> 2)), DLW_TAG, k0, k1, x);
            const int s4 = lane & 3;
            const uint32_t w = s4 == 0 ? x[0] : s4 == 1 ? x[1] : s4 == 2 ? x[2] : x[3];
            const uint32_t rr = __umulhi(w, T);                                    // < T
            uint32_t lo = 0u, hi = U - 1u;                                         // the answer lies in [lo, hi]
            for (int s = 0; s < steps; ++s) {                                      // hi - lo at least halves: bits(U - 1) steps
                const uint32_t mid = lo + ((hi - lo) >> 1);                        // <= U - 1 always; < hi while lo < hi
                const uint32_t v = cdf[mid];
                const bool open = lo < hi, up = v <= rr;
                lo = open && up ? mid + 1u : lo;
                hi = open && !up ? mid : hi;
            }
            const uint32_t j = lo;
            bool ok = j != (uint32_t)a;
            const uint4* acc4 = reinterpret_cast<const uint4*>(acc);
            for (int s = 0; 4 * s < cnt; ++s) {                                    // 4 s + 3 < W
                const uint4 e = acc4[s];
                ok = ok && e.x != j && e.y != j && e.z != j && e.w != j;
            }
            unsigned long long walk = __ballot(ok);
            while (walk) {                                                         // earliest lane first
                const int l = __ffsll(walk) - 1;
                walk &= walk - 1ull;
                const uint32_t jl = __builtin_amdgcn_readlane(j, l);
                if (lane > l && jl == j) ok = false;
            }
            const unsigned long long won = __ballot(ok);
            const int slot = cnt + __popcll(won & ((1ull << lane) - 1ull));
            if (ok && slot < m) acc[slot] = j;
            cnt = min(m, cnt + __popcll(won));
            dl_wave_fence();
        }
    }
    if (cnt < m) {                                       // wave-uniform: no target, T == 0, or incomplete at the cap
        if (lists_out)
            for (int p = lane; p < Lg; p += 64) lists_out[o + p] = -1;
        if (tuples_out)
            for (int e = lane; e < Lg * nf; e += 64) tuples_out[o * nf + e] = 0;
        if (lane == 0) target_out[g] = -1;
        return;
    }
    uint32_t xp[4];
    philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), DLW_PLACE, DLW_TAG, k0, k1, xp);
    const int place = (int)__umulhi(xp[0], (uint32_t)Lg);
    for (int p = lane; p < Lg; p += 64) {
        const uint32_t v = p == place ? (uint32_t)a : acc[p - (p > place ? 1 : 0)];    // an index in [0, m)
        key[p] = v;
        if (lists_out) lists_out[o + p] = (int32_t)v;
    }
    if (lane == 0) target_out[g] = place;
    if (tuples_out) {
        dl_wave_fence();
        for (int e = lane; e < Lg * nf; e += 64) {
            const int p = e / nf, c = e - p * nf;
            tuples_out[o * nf + e] = cand[(int64_t)key[p] * nf + c];              // key[p] < U
        }
    }
}

extern "C" int cffm_draw_lists_weighted(uint64_t seed, int64_t list0, int32_t G, const int32_t* at, int32_t U, int32_t m,
                                        const uint32_t* cdf, const int32_t* cand, int32_t nf, int32_t* lists_out, int32_t* tuples_out,
                                        int32_t* target_out, void* stream) {
    if (U < 1 || !cdf || !draw_args_ok(list0, G, at, U, m, cand, nf, lists_out, tuples_out, target_out)) return CFFM_ERR_BAD_SHAPE;
    if (G == 0) return 0;
    const int W = (m + 1 + 3) & ~3;
    const size_t lds = (size_t)DL_WAVES * 2 * W * sizeof(uint32_t);                // at most 32 KiB
    const int nb = (G + DL_WAVES - 1) / DL_WAVES;
    int steps = 0;                                                                 // bits(U - 1)
    for (uint32_t n = (uint32_t)U - 1u; n; n >>= 1) ++steps;
    const int rounds = 8 * ((m + 1 + 63) / 64) + 8;                                // the word cap, in rounds of 64
    hipLaunchKernelGGL(draw_lists_weighted_kernel, dim3(nb), dim3(64 * DL_WAVES), lds, (hipStream_t)stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint64_t)list0, G, at, (uint32_t)U, m, W, steps, rounds, cdf, cand, nf, lists_out,
                       tuples_out, target_out);
    CFFM_CHECK_LAUNCH();
    return 0;
}
