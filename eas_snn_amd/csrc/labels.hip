// The label side of a training sample on the device (eas_label_targets): the box half of GEN1Dataset.get_random_data
// (yolox/data/datasets/gen1.py:437, 459-468, 510-521; rvt_gen4.py:510-598 and ncaltech.py:272-366 are the same arithmetic), reformat('cxcywh')
// (yolox/utils/boxes.py:131-136) and EventTrainTransform.__call__ (yolox/data/event_data_augment.py:19-65) for a batch, from a box table that
// stays in HBM.
//   boxes        f32 [L][5]      (x1, y1, x2, y2, class) on the sensor, the rows of label group g at group_start[g] .. group_start[g + 1]
//   targets      f32 [B][max_labels][5]   (class, cx, cy, w, h) of the boxes that survive the resize / paste / flip / clip, in their (shuffled)
//                                order, zero rows behind them: every element is written
// One wavefront per sample.  Its lanes walk the sample's shuffled list in chunks of 64 rows; a kept row goes to position (rows kept in earlier
// chunks) + (kept lanes below this one: ballot + popcount), which preserves the order across chunks.  Integer work and one IEEE double division
// per coordinate: bit-exact.  Everything read through device data is bounded: the group index by G, the row range by L, a perm entry by the
// group's row count.
#include "eas_common.h"

namespace {

constexpr int kWavesPerBlock = EAS_BLOCK / EAS_WAVE;

// one coordinate through resize and paste: the product in integers, one double division, one addition, truncation toward zero
// (numpy: int64 array * int / int + int, stored back into the int64 array)
__device__ __forceinline__ int64_t resize_coord(int64_t v, int n_new, int n_old, int shift) {
    return (int64_t)((double)(v * (int64_t)n_new) / (double)n_old + (double)shift);
}

__global__ __launch_bounds__(EAS_BLOCK) void label_targets_kernel(const float* __restrict__ boxes, int64_t L, const int64_t* __restrict__ group_start,
                                                                  int G, const int64_t* __restrict__ group, const int32_t* __restrict__ params,
                                                                  const int32_t* __restrict__ perm, int P, int B, int ih, int iw, int h, int w,
                                                                  int max_labels, float* __restrict__ targets, int32_t* __restrict__ count,
                                                                  int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & (EAS_WAVE - 1);
    const int b = blockIdx.x * kWavesPerBlock + threadIdx.x / EAS_WAVE;
    if (b >= B) return;                                        // wave-uniform: the ballots below see whole waves
    const int64_t g = group[b];
    const bool bad_group = g < 0 || g >= (int64_t)G;
    int64_t row0 = 0, n = 0;
    if (!bad_group) {
        int64_t row1 = group_start[g + 1];
        row0 = group_start[g];
        row0 = row0 < 0 ? 0 : (row0 > L ? L : row0);           // a table that does not describe `boxes` never leads outside of it
        row1 = row1 < row0 ? row0 : (row1 > L ? L : row1);
        n = row1 - row0;
    }
    const int64_t listed = perm ? (n < (int64_t)P ? n : (int64_t)P) : n;      // rows of the shuffled list
    const int32_t* par = params + 5 * (int64_t)b;
    const int nw = par[0], nh = par[1], dx = par[2], dy = par[3];
    const bool flip = par[4] != 0;
    float* out = targets + (int64_t)b * max_labels * 5;

    int64_t kept = 0;                                          // survivors so far (wave-uniform)
    bool bad_perm = false;
    for (int64_t j0 = 0; j0 < listed; j0 += EAS_WAVE) {
        const int64_t j = j0 + lane;
        bool keep = false;
        int64_t x1 = 0, y1 = 0, x2 = 0, y2 = 0, cls = 0;
        if (j < listed) {
            const int64_t r = perm ? (int64_t)perm[(int64_t)b * P + j] : j;
            if (r < 0 || r >= n) {
                bad_perm = true;
            } else {
                const float* row = boxes + (row0 + r) * 5;
                x1 = resize_coord((int64_t)row[0], nw, iw, dx);
                y1 = resize_coord((int64_t)row[1], nh, ih, dy);
                x2 = resize_coord((int64_t)row[2], nw, iw, dx);
                y2 = resize_coord((int64_t)row[3], nh, ih, dy);
                cls = (int64_t)row[4];
                if (flip) {
                    const int64_t left = (int64_t)w - x2;
                    x2 = (int64_t)w - x1;
                    x1 = left;
                }
                x1 = x1 < 0 ? 0 : x1;
                y1 = y1 < 0 ? 0 : y1;
                x2 = x2 > w ? (int64_t)w : x2;
                y2 = y2 > h ? (int64_t)h : y2;
                keep = x2 - x1 > 1 && y2 - y1 > 1;
            }
        }
        const unsigned long long mask = __ballot(keep);
        const int64_t pos = kept + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && pos < max_labels) {
            const float fx1 = (float)x1, fy1 = (float)y1;
            const float bw = (float)x2 - fx1, bh = (float)y2 - fy1;
            float* t = out + pos * 5;
            t[0] = (float)cls;
            t[1] = fx1 + bw * 0.5f;
            t[2] = fy1 + bh * 0.5f;
            t[3] = bw;
            t[4] = bh;
        }
        kept += __popcll(mask);
    }
    // the zero rows behind the survivors
    const int64_t filled = (kept < max_labels ? kept : (int64_t)max_labels) * 5;
    for (int64_t i = filled + lane; i < (int64_t)max_labels * 5; i += EAS_WAVE) out[i] = 0.f;
    const bool any_bad_perm = __ballot(bad_perm) != 0ull;
    if (lane == 0) {
        if (count) count[b] = (int32_t)(kept > INT32_MAX ? INT32_MAX : kept);
        if (flags) flags[b] = (any_bad_perm ? 1 : 0) | ((perm && n > (int64_t)P) ? 2 : 0) | (bad_group ? 4 : 0);
    }
}

}  // namespace

extern "C" int eas_label_targets(const float* boxes, int64_t L, const int64_t* group_start, int G, const int64_t* group, const int32_t* params,
                                 const int32_t* perm, int P, int B, int ih, int iw, int h, int w, int max_labels, float* targets, int32_t* count,
                                 int32_t* flags, eas_stream_t stream) {
    if (L < 0 || G < 0 || B < 0 || P < 0 || max_labels < 1 || ih < 1 || iw < 1) return EAS_ERR_INVALID_ARG;
    if ((((uintptr_t)group_start | (uintptr_t)group) & 7) ||
        (((uintptr_t)boxes | (uintptr_t)params | (uintptr_t)perm | (uintptr_t)targets | (uintptr_t)count | (uintptr_t)flags) & 3))
        return EAS_ERR_INVALID_ARG;
    if (B == 0) return EAS_OK;                                 // an empty batch has no per-sample arrays: their pointers may be NULL
    if (!group_start || !group || !params || !targets || (!boxes && L != 0)) return EAS_ERR_INVALID_ARG;
    const int blocks = (B + kWavesPerBlock - 1) / kWavesPerBlock;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(label_targets_kernel, dim3(blocks), dim3(EAS_BLOCK), 0, eas_s(stream), boxes, L, group_start, G, group, params, perm, P, B, ih, iw, h,
               w, max_labels, targets, count, flags);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}
