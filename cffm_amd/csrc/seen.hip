// The skip mask of a ranking call made on the device from a sparse "seen" relation (cffm_seen_mask, include/cffm_hip.h, DESIGN.md
// 3.6.4): context c owns CSR row row[c] of (off, pos), every entry a candidate POSITION of the call, and byte (c, n) of the mask is 1
// where n is among them or where the caller's own mask skip_in is non-zero there.  The mask is what cffm_topk and cffm_rank_of take as
// `skip`; cffm_amd/spec.py seen_mask() is the numpy twin and the specification, malformed relations included.
//
// One workgroup of 256 threads per (context, chunk of 4096 positions) unit, the units flattened over a 1-D grid in 64 bits (C may
// exceed what grid.y holds) and walked grid-stride where there are more units than SEEN_MAX_GRID.  Per unit:
//   1. the chunk's bytes are formed in an LDS tile: zeros, or the bytes of skip_in normalised to 0 / 1
//   2. barrier; all threads stride over the context's [lo, hi) range of pos (coalesced int32 loads) and an entry inside the chunk
//      stores the byte 1 into the tile - the same value from whoever stores it, so repeats and races between them are benign
//   3. barrier; the tile goes out
//   4. barrier, before the next unit of the walk fills the tile again
// The tile sits in LDS at the offset a = (address of the chunk's first output byte) mod 16, so a 16-byte slot of the LDS is a 16-byte
// ALIGNED piece of the output whatever mask_stride is: a slot that lies wholly inside the chunk leaves as one vector store, the
// ragged slot at the head and the one at the tail as bytes.  skip_in comes in the same way where its chunk has the same a (two
// contiguous [C][N] buffers always do), and byte by byte, 64 consecutive bytes per wavefront, where it does not.
// No atomics, no global read-modify-write, every output byte stored exactly once (a dirty buffer ends as a clean one does), and the
// three barriers sit at the top level of a loop whose trip count depends on blockIdx and gridDim alone.
// Nothing read from the device steers an address out of its array: row[c] is tested against [0, R) before off is read, both offsets
// are clamped into [0, nnz], a decreasing pair gives an empty range, and an entry of pos is a tile index only inside the chunk.
#include "internal.hpp"

#define SEEN_CHUNK 4096
#define SEEN_THREADS 256
#define SEEN_SLOTS (SEEN_CHUNK / 16 + 1)        // 16-byte slots of the tile: the chunk shifted by up to 15 bytes
#define SEEN_MAX_GRID (1 << 14)

namespace {

// every non-zero byte of w becomes 1
__device__ __forceinline__ uint32_t seen_norm(uint32_t w) {
    w |= w >> 4;                                 // bits 0..3 of a byte now hold its own two nibbles, or-ed
    w |= w >> 2;
    w |= w >> 1;
    return w & 0x01010101u;
}

__global__ __launch_bounds__(SEEN_THREADS) void seen_mask_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ pos, int R,
                                                                 int64_t nnz, const int32_t* __restrict__ row,
                                                                 const uint8_t* __restrict__ skip_in, int64_t skip_in_stride, int N,
                                                                 int chunks, int64_t units, uint8_t* __restrict__ mask_out,
                                                                 int64_t mask_stride) {
    __shared__ uint4 tile4[SEEN_SLOTS];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tile4);
    const int tid = threadIdx.x;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t c = u / chunks;
        const int64_t n0 = (u - c * chunks) * SEEN_CHUNK;
        const int len = (int)(N - n0 < SEEN_CHUNK ? N - n0 : SEEN_CHUNK);          // 1 .. 4096 positions of this chunk
        uint8_t* dst = mask_out + c * mask_stride + n0;
        const int a = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
        const int slots = (a + len + 15) >> 4;                                     // <= SEEN_SLOTS
        // 1. tile byte a + i is position n0 + i
        const uint8_t* src = skip_in ? skip_in + c * skip_in_stride + n0 : nullptr;
        if (src && (int)(reinterpret_cast<uintptr_t>(src) & 15) != a) {
            for (int i = tid; i < len; i += SEEN_THREADS) tile[a + i] = src[i] ? 1 : 0;
        } else {
            for (int s = tid; s < slots; s += SEEN_THREADS) {
                const int b = s * 16 - a;                                          // chunk byte of the slot's first byte
                if (!src) {
                    tile4[s] = make_uint4(0u, 0u, 0u, 0u);
                } else if (b >= 0 && b + 16 <= len) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + b);      // 16-byte aligned: src = a (mod 16)
                    tile4[s] = make_uint4(seen_norm(v.x), seen_norm(v.y), seen_norm(v.z), seen_norm(v.w));
                } else {
                    const int i0 = b < 0 ? 0 : b, i1 = b + 16 < len ? b + 16 : len;
                    for (int i = i0; i < i1; ++i) tile[a + i] = src[i] ? 1 : 0;
                }
            }
        }
        __syncthreads();
        // 2. the context's entries
        const int r = row[c];
        if (r >= 0 && r < R) {
            int64_t lo = off[r], hi = off[r + 1];
            lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
            hi = hi < 0 ? 0 : (hi > nnz ? nnz : hi);
            for (int64_t j = lo + tid; j < hi; j += SEEN_THREADS) {                // empty where hi <= lo
                const int64_t i = (int64_t)pos[j] - n0;
                if (i >= 0 && i < len) tile[a + i] = 1;
            }
        }
        __syncthreads();
        // 3. out: whole slots as aligned vectors, the head and the tail as bytes
        for (int s = tid; s < slots; s += SEEN_THREADS) {
            const int b = s * 16 - a;
            if (b >= 0 && b + 16 <= len) {
                *reinterpret_cast<uint4*>(dst + b) = tile4[s];
            } else {
                const int i0 = b < 0 ? 0 : b, i1 = b + 16 < len ? b + 16 : len;
                for (int i = i0; i < i1; ++i) dst[i] = tile[a + i];
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int cffm_seen_mask(const int32_t* off, const int32_t* pos, int32_t R, int64_t nnz, const int32_t* row, const uint8_t* skip_in,
                              int64_t skip_in_stride, int32_t C, int32_t N, uint8_t* mask_out, int64_t mask_stride, void* stream) {
    if (!off || !row || !mask_out || (!pos && nnz != 0)) return CFFM_ERR_BAD_SHAPE;
    if (N < 1 || C < 0 || R < 0 || nnz < 0) return CFFM_ERR_BAD_SHAPE;
    if (mask_stride < N) return CFFM_ERR_BAD_SHAPE;
    if (skip_in && skip_in_stride < N) return CFFM_ERR_BAD_SHAPE;
    if (skip_in == mask_out) return CFFM_ERR_BAD_SHAPE;
    if (C == 0) return 0;
    const int chunks = (int)(((int64_t)N + SEEN_CHUNK - 1) / SEEN_CHUNK);
    const int64_t units = (int64_t)C * chunks;                                     // < 2^31 * 2^19
    const unsigned grid = (unsigned)(units < SEEN_MAX_GRID ? units : SEEN_MAX_GRID);
    hipLaunchKernelGGL(seen_mask_kernel, dim3(grid), dim3(SEEN_THREADS), 0, (hipStream_t)stream, off, pos, (int)R, nnz, row, skip_in,
                       skip_in_stride, (int)N, chunks, units, mask_out, mask_stride);
    CFFM_CHECK_LAUNCH();
    return 0;
}
