// Hard negatives picked from a scored pool, BY LIST ID (cffm_pick_hard, include/cffm_hip.h): list g of a call has
// the id list0 + g; from the Lp scored pool positions of the list - its positive at target_pool[g], Lp - 1 negatives - the m
// best-scored negatives in THE ORDER of rank.hip (rank_key.hpp: score descending, -0 == +0, NaN below -inf, equal scores to the
// smaller position) become the list's negatives, hardest first, around the positive at a drawn place.  cffm_amd/spec.py pick_hard()
// is the numpy twin and the specification; everything here is integer arithmetic on the scores' bits and matches it exactly.
//
//   rank    of a negative = the number of negatives with a larger key.  The keys are distinct (the position is their low word), so
//           the ranks of the Lp - 1 negatives are a permutation of 0 .. Lp - 2; the positive's key is taken as 0, which no pool
//           position has and nothing is smaller than, so it is counted by nobody
//   place   (w * (m + 1)) >> 32 with w = output word 0 of Philox4x32-10 at counter (id lo, id hi, 0, 4), key seed: a function of
//           (seed, id, m) alone.  The negative of rank r < m goes to slot r + (r >= place)
//
// The layout of draw.hip: one wavefront per list, four lists per workgroup, and NO workgroup barrier - a wavefront past the last list
// returns at once and the others never wait for it.  A wavefront forms its Lp keys once into its own slice of the dynamic LDS (8 Lp
// bytes, at most 8 KiB) and keeps the slot -> pool position map in a second slice (m + 1 words).  Selection is by rank counting, no
// sort: lane l owns the positions l, l + 64, ...; for one of them at a time it counts over j = 0 .. Lp - 1 while every lane reads
// key j at the same address (a broadcast).  Lp * ceil(Lp / 64) 64-bit compares per lane, every trip count and branch wave-uniform.
// Same-wavefront LDS traffic is ordered by wavefront-scope fences.  The map goes through LDS so that the gather of the pool rows and
// the stores run coalesced over (slot, a).
#include "internal.hpp"
#include "philox.hpp"
#include "rank_key.hpp"

#define PH_WAVES 4        // lists per workgroup
#define PH_TAG 4u         // the pick's value of the fourth counter word (table draw 0 and 1, list draws 2 and 3)
#define PH_MAX_LP 1024

namespace {

__device__ __forceinline__ void ph_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64 * PH_WAVES) void pick_hard_kernel(uint32_t k0, uint32_t k1, uint64_t list0, int G,
                                                                  const unsigned* __restrict__ sbits, int64_t row_stride, int Lp,
                                                                  const int32_t* __restrict__ target_pool, int m, int W,
                                                                  const int32_t* __restrict__ pool_lists,
                                                                  const int32_t* __restrict__ pool_tuples, int nf,
                                                                  int32_t* __restrict__ lists_out, int32_t* __restrict__ tuples_out,
                                                                  int32_t* __restrict__ target_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ph_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * PH_WAVES + wave;
    if (g >= G) return;                                  // wave-uniform; nothing below waits for another wavefront
    unsigned long long* key = ph_lds + (size_t)wave * Lp;                                    // 8-byte aligned
    uint32_t* sel = reinterpret_cast<uint32_t*>(ph_lds + (size_t)PH_WAVES * Lp) + (size_t)wave * W;   // slot -> pool position
    const int Lg = m + 1;
    const int64_t o = (int64_t)g * Lg;
    const int32_t t = target_pool[g];
    if (t < 0 || t >= Lp) {                              // defined: no target, an index row of -1, a tuple row of zeros
        if (lists_out)
            for (int p = lane; p < Lg; p += 64) lists_out[o + p] = -1;
        if (tuples_out)
            for (int e = lane; e < Lg * nf; e += 64) tuples_out[o * nf + e] = 0;
        if (lane == 0) target_out[g] = -1;
        return;
    }
    const unsigned* srow = sbits + (int64_t)g * row_stride;
    for (int p = lane; p < Lp; p += 64) key[p] = p == t ? 0ull : rank_key64(srow[p], (unsigned)p);
    const uint64_t id = list0 + (uint64_t)g;
    uint32_t x[4];
    philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), 0u, PH_TAG, k0, k1, x);
    const int place = (int)__umulhi(x[0], (uint32_t)Lg);                                     // 0 <= place <= m
    ph_wave_fence();
    for (int e0 = 0; e0 < Lp; e0 += 64) {
        const int e = e0 + lane;
        const unsigned long long mine = e < Lp ? key[e] : ~0ull;                             // nothing beats a lane past the pool
        int r = 0;
#pragma unroll 4
        for (int j = 0; j < Lp; ++j) r += key[j] > mine ? 1 : 0;                             // the same address in every lane
        if (e < Lp && e != t && r < m) sel[r + (r >= place ? 1 : 0)] = (uint32_t)e;         // a slot of [0, m], each written once
    }
    if (lane == 0) {
        sel[place] = (uint32_t)t;
        target_out[g] = place;
    }
    ph_wave_fence();
    const int64_t po = (int64_t)g * Lp;
    if (lists_out)
        for (int p = lane; p < Lg; p += 64) lists_out[o + p] = pool_lists[po + sel[p]];     // sel[p] < Lp
    if (tuples_out)
        for (int e = lane; e < Lg * nf; e += 64) {
            const int p = e / nf, c = e - p * nf;
            tuples_out[o * nf + e] = pool_tuples[(po + sel[p]) * nf + c];
        }
}

}  // namespace

extern "C" int cffm_pick_hard(uint64_t seed, int64_t list0, int32_t G, const float* scores, int64_t row_stride, int32_t Lp,
                              const int32_t* target_pool, int32_t m, const int32_t* pool_lists, const int32_t* pool_tuples, int32_t nf,
                              int32_t* lists_out, int32_t* tuples_out, int32_t* target_out, void* stream) {
    if (Lp < 2 || Lp > PH_MAX_LP || m < 1 || m > Lp - 1 || G < 0 || list0 < 0 || list0 > INT64_MAX - (int64_t)G || nf < 0 ||
        row_stride < Lp)
        return CFFM_ERR_BAD_SHAPE;
    const int64_t slots = (int64_t)G * Lp;                                                   // < 2^41
    if (slots >= (1ll << 31) || slots * (nf > 1 ? nf : 1) >= (1ll << 31)) return CFFM_ERR_BAD_SHAPE;
    if ((pool_tuples == nullptr) != (tuples_out == nullptr) || (pool_lists == nullptr) != (lists_out == nullptr)) return CFFM_ERR_BAD_SHAPE;
    if (nf == 0 && pool_tuples) return CFFM_ERR_BAD_SHAPE;
    if (!lists_out && !tuples_out) return CFFM_ERR_BAD_SHAPE;
    if (!scores || !target_pool || !target_out) return CFFM_ERR_BAD_SHAPE;
    if (G == 0) return 0;
    const int W = (m + 1 + 3) & ~3;
    const size_t lds = (size_t)PH_WAVES * ((size_t)Lp * sizeof(unsigned long long) + (size_t)W * sizeof(uint32_t));   // at most 48 KiB
    const int nb = (G + PH_WAVES - 1) / PH_WAVES;
    hipLaunchKernelGGL(pick_hard_kernel, dim3(nb), dim3(64 * PH_WAVES), lds, (hipStream_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint64_t)list0, G, (const unsigned*)scores, row_stride, (int)Lp, target_pool, (int)m, W, pool_lists, pool_tuples,
                       (int)nf, lists_out, tuples_out, target_out);
    CFFM_CHECK_LAUNCH();
    return 0;
}
