// A 128-bit digest of a device buffer in one reading pass (eas_bytes_digest; include/eas_hip.h states the definition): what a store
// snapshot (data._Store.save / data.load_store) is checked by after its bytes are back in HBM, where a pass over them costs a fraction of
// what a host hash of the same bytes would.
//
// IT IS A CORRUPTION CHECK, NOT A CRYPTOGRAPHIC HASH.  Truncation, bit flips and swapped words change it; somebody who wants two buffers
// with one digest can construct them.
//
// The buffer is read as little-endian 64-bit words q_0 .. q_{n-1} (the missing bytes of the last word are zero); word i is mixed with its
// index by the splitmix64 finalizer,
//     z = q_i + (i + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
// and out2 = (sum of all z mod 2^64, xor of all z).  Both are order-independent, so the words may be dealt to lanes, waves and blocks in any
// way and the result is the same bits in every run: per-lane sum and xor, a wave reduction, a block reduction, one 64-bit atomicAdd and one
// atomicXor per block.  A lane takes two words per 16-byte load; the grid is a fixed number of blocks per CU and strides over the pairs;
// the odd full word and the partial last word (formed from byte loads) are lane 0 of block 0's.
#include "eas_common.h"

namespace {

constexpr int kDigestBlocksPerCU = 4;                       // 16 waves per CU: with the loop's loads in flight enough to cover HBM latency
constexpr int kDigestBlocks = 256 * kDigestBlocksPerCU;     // the 256 CUs of the chip; never a function of nbytes
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// the mixed word: q + g with g = (index + 1) * kGolden, then the finalizer
__device__ __forceinline__ uint64_t digest_mix(uint64_t q, uint64_t g) {
    uint64_t z = q + g;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t wave_xor(uint64_t v) {
#pragma unroll
    for (int off = EAS_WAVE / 2; off > 0; off >>= 1) v ^= (uint64_t)__shfl_down((unsigned long long)v, off, EAS_WAVE);
    return v;  // valid in lane 0
}

__global__ __launch_bounds__(EAS_BLOCK) void bytes_digest_kernel(const uint8_t* __restrict__ buf, int64_t nbytes,
                                                                 unsigned long long* __restrict__ out2) {
    const int64_t full = nbytes >> 3;                       // whole words
    const int64_t pairs = full >> 1;                        // 16-byte loads
    const ulonglong2* __restrict__ p = reinterpret_cast<const ulonglong2*>(buf);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t g = (uint64_t)(2 * i + 1) * kGolden;           // (index + 1) * kGolden of word 2 i, moved on by additions
    const uint64_t dg = (uint64_t)(2 * stride) * kGolden;
    uint64_t s = 0, x = 0;
#pragma unroll 4
    for (; i < pairs; i += stride, g += dg) {
        const ulonglong2 v = p[i];
        const uint64_t z0 = digest_mix(v.x, g), z1 = digest_mix(v.y, g + kGolden);
        s += z0 + z1;
        x ^= z0 ^ z1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (full & 1) {                                     // the full word behind the last pair
            const uint64_t z = digest_mix(reinterpret_cast<const unsigned long long*>(buf)[full - 1], (uint64_t)full * kGolden);
            s += z;
            x ^= z;
        }
        const int rest = (int)(nbytes & 7);
        if (rest) {                                         // the partial last word: its missing bytes are zero
            uint64_t q = 0;
            for (int b = 0; b < rest; ++b) q |= (uint64_t)buf[full * 8 + b] << (8 * b);
            const uint64_t z = digest_mix(q, (uint64_t)(full + 1) * kGolden);
            s += z;
            x ^= z;
        }
    }
    __shared__ unsigned long long red[2][EAS_BLOCK / EAS_WAVE];
    s = eas_wave_sum((unsigned long long)s);
    x = wave_xor(x);
    if ((threadIdx.x & (EAS_WAVE - 1)) == 0) {
        red[0][threadIdx.x / EAS_WAVE] = s;
        red[1][threadIdx.x / EAS_WAVE] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0;
        x = 0;
#pragma unroll
        for (int w = 0; w < EAS_BLOCK / EAS_WAVE; ++w) {
            s += red[0][w];
            x ^= red[1][w];
        }
        if (s) atomicAdd(out2, (unsigned long long)s);      // (a block without words adds nothing)
        if (x) atomicXor(out2 + 1, (unsigned long long)x);
    }
}

}  // namespace

extern "C" int eas_bytes_digest(const void* buf, long long nbytes, unsigned long long* out2, eas_stream_t stream) {
    if (nbytes < 0 || nbytes > (1ll << 40) || !out2 || ((uintptr_t)out2 & 7)) return EAS_ERR_INVALID_ARG;
    if (nbytes > 0 && (!buf || ((uintptr_t)buf & 15))) return EAS_ERR_INVALID_ARG;
    EAS_CLEAR_ERR();
    if (hipMemsetAsync(out2, 0, 2 * sizeof(unsigned long long), eas_s(stream)) != hipSuccess) return EAS_ERR_LAUNCH;
    if (nbytes == 0) return EAS_OK;
    EAS_LAUNCH(bytes_digest_kernel, dim3(kDigestBlocks), dim3(EAS_BLOCK), 0, eas_s(stream), static_cast<const uint8_t*>(buf), (int64_t)nbytes, out2);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}
