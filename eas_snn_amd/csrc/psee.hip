// Prophesee-protocol front half of the AP evaluation on the device: box filter, time matching and the expansion into the flat
// (image, category, box, score) rows that eas_cocoeval_* take (reference: yolox/utils/psee_loader/evaluation.py:6-43 evaluate_list,
// io/box_filtering.py:23-41 filter_boxes, metrics/coco_eval.py:25-91 evaluate_detection / _match_times, :128-179 _to_coco_format).
//
// A box set is (t int64 [N], box float32 [N][4] = x, y, w, h, cls int32 [N], score float32 [N] for detections, file_offsets int64 [F+1]):
// the rows of file f are [file_offsets[f], file_offsets[f+1]), ascending in t.  Both sets have the same F files.
//
// Calls; the prefix sums between them are the caller's (int64, any inclusive / exclusive scan):
//   mark     one thread per row: keep = (t > skip_ts) && (w*w + h*h >= diag*diag) && (w >= side) && (h >= side), float32 with every product
//            and the sum rounded on its own (__fmul_rn / __fadd_rn: never contracted to an fma), the thresholds converted to float32 as
//            numpy converts the Python integers.  For ground truths also first = kept and no earlier kept row of the file has the same t:
//            one image per first flag, numbered by the scan of the flags (files in order, then ascending t: the order of np.unique).
//   [scans]  gt_keep_scan [Ng+1] and dt_keep_scan [Nd+1] exclusive (entry N = the total), gt_img_scan [Ng] inclusive over first
//   windows  one thread per ground-truth row.  A kept row counts itself into pair_count[image * K + cls] (integer atomics: the largest
//            entry is what eas_cocoeval_supported asks for).  A first row writes its image: file, t, and the window of the file's kept
//            detections with ts - tol <= t <= ts + tol: lower / upper bound over the file's rows in int64 (what the reference's two-pointer
//            walk arrives at, the rows ascending), turned into positions among ALL kept detections by dt_keep_scan -- filtering keeps the
//            order and the window is a predicate on t alone, so the kept rows between the two bounds are the window of the filtered array.
//   [scan]   det_off [Ng+1] exclusive over win_cnt (entries behind the last image are 0); det_off[I] = D, the expanded detection rows:
//            a detection is copied into every image whose window holds it.  I, D, G come back to the host here -- the one read.
//   expand   one thread per output row.  Ground truths: the kept rows in order (that IS image-major: images ascend with the rows),
//            gt_id = position + 1 (annotation ids 1..G, _to_coco_format :159).  Detections: row d belongs to image i = the last one
//            with det_off[i] <= d, and is kept detection number win_lo[i] + d - det_off[i], whose source row is the last s with
//            dt_keep_scan[s] <= that number.
//
// Every index is int64; indices read from device arrays are clamped into their tables before use, so offsets or sizes that do not belong
// to the data give wrong rows, never an access outside the arrays.  Zero rows, zero files and "nothing kept" launch nothing.
#include "eas_common.h"

namespace {

// first index in [lo, hi) with a[index] >= v
__device__ __forceinline__ long long ps_lower_bound(const long long* __restrict__ a, long long lo, long long hi, long long v) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// first index in [lo, hi) with a[index] > v
__device__ __forceinline__ long long ps_upper_bound(const long long* __restrict__ a, long long lo, long long hi, long long v) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long long ps_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the file whose range holds row r: the last f in [0, F) with offsets[f] <= r (empty files share their offset with the next one)
__device__ __forceinline__ long long ps_file_of(const long long* __restrict__ offsets, long long F, long long r) {
    return ps_clamp(ps_upper_bound(offsets, 0, F + 1, r) - 1, 0, F - 1);
}

struct PsFilter {
    long long skip_ts;
    float diag2, side;
    int apply;
};

__device__ __forceinline__ bool ps_keep(const PsFilter& f, long long t, const float* __restrict__ box) {
    if (!f.apply) return true;
    const float w = box[2], h = box[3];
    const float d2 = __fadd_rn(__fmul_rn(w, w), __fmul_rn(h, h));
    return t > f.skip_ts && d2 >= f.diag2 && w >= f.side && h >= f.side;
}

__global__ __launch_bounds__(EAS_BLOCK) void ps_mark_kernel(const long long* __restrict__ t, const float* __restrict__ box, long long N,
                                                            const long long* __restrict__ offsets, long long F, PsFilter f,
                                                            int* __restrict__ keep, int* __restrict__ first) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += stride) {
        const long long ts = t[r];
        const bool k = ps_keep(f, ts, box + r * 4);
        keep[r] = k ? 1 : 0;
        if (first) {
            bool is_first = k;
            if (k) {
                const long long start = ps_clamp(offsets[ps_file_of(offsets, F, r)], 0, r);
                for (long long q = r - 1; q >= start && t[q] == ts; --q)
                    if (ps_keep(f, ts, box + q * 4)) { is_first = false; break; }
            }
            first[r] = is_first ? 1 : 0;
        }
    }
}

struct PsWindows {
    const long long* gt_t;            // [Ng]
    const int* gt_cls;                // [Ng]
    const int* gt_keep;               // [Ng]
    const int* gt_first;              // [Ng]
    const long long* gt_img_scan;     // [Ng] inclusive scan of gt_first
    const long long* gt_offsets;      // [F+1]
    const long long* dt_t;            // [Nd]
    const long long* dt_offsets;      // [F+1]
    const long long* dt_keep_scan;    // [Nd+1] exclusive scan of the detections' keep flags
    long long Ng, Nd, F, tol;
    int K;
    int* image_file;                  // [Ng] the first I are written
    long long* image_t;               // [Ng]
    long long* win_lo;                // [Ng]
    long long* win_cnt;               // [Ng] zeroed before the launch
    int* pair_count;                  // [Ng][K] zeroed before the launch
};

__global__ __launch_bounds__(EAS_BLOCK) void ps_windows_kernel(PsWindows p) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < p.Ng; r += stride) {
        if (!p.gt_keep[r]) continue;
        const long long i = ps_clamp(p.gt_img_scan[r] - 1, 0, p.Ng - 1);
        const int c = p.gt_cls[r];
        if (c >= 0 && c < p.K) atomicAdd(&p.pair_count[i * p.K + c], 1);
        if (!p.gt_first[r]) continue;
        const long long f = ps_file_of(p.gt_offsets, p.F, r);
        const long long ts = p.gt_t[r];
        p.image_file[i] = (int)f;
        p.image_t[i] = ts;
        const long long a = ps_clamp(p.dt_offsets[f], 0, p.Nd), b = ps_clamp(p.dt_offsets[f + 1], a, p.Nd);
        const long long lo = ps_lower_bound(p.dt_t, a, b, ts - p.tol), hi = ps_upper_bound(p.dt_t, lo, b, ts + p.tol);
        const long long k0 = p.dt_keep_scan[lo], k1 = p.dt_keep_scan[hi];
        p.win_lo[i] = k0;
        p.win_cnt[i] = k1 > k0 ? k1 - k0 : 0;
    }
}

__global__ __launch_bounds__(EAS_BLOCK) void ps_expand_gt_kernel(const int* __restrict__ keep, const long long* __restrict__ keep_scan,
                                                                 const long long* __restrict__ img_scan, const int* __restrict__ cls,
                                                                 const float* __restrict__ box, long long N, long long G,
                                                                 int* __restrict__ out_img, int* __restrict__ out_cls,
                                                                 float* __restrict__ out_box, long long* __restrict__ out_id) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += stride) {
        if (!keep[r]) continue;
        const long long g = keep_scan[r];
        if (g < 0 || g >= G) continue;
        out_img[g] = (int)(img_scan[r] - 1);
        out_cls[g] = cls[r];
        out_id[g] = g + 1;
        for (int k = 0; k < 4; ++k) out_box[g * 4 + k] = box[r * 4 + k];
    }
}

struct PsExpandDet {
    const long long* det_off;         // [>= I+1] exclusive scan of win_cnt
    const long long* win_lo;          // [I]
    const long long* keep_scan;       // [Nd+1]
    const int* cls;                   // [Nd]
    const float* box;                 // [Nd][4]
    const float* score;               // [Nd]
    long long I, D, Nd;
    int* out_img;                     // [D]
    int* out_cls;
    float* out_box;
    float* out_score;
};

__global__ __launch_bounds__(EAS_BLOCK) void ps_expand_det_kernel(PsExpandDet p) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x; d < p.D; d += stride) {
        const long long i = ps_clamp(ps_upper_bound(p.det_off, 0, p.I + 1, d) - 1, 0, p.I - 1);
        const long long number = p.win_lo[i] + (d - p.det_off[i]);
        const long long s = ps_clamp(ps_upper_bound(p.keep_scan, 0, p.Nd + 1, number) - 1, 0, p.Nd - 1);
        p.out_img[d] = (int)i;
        p.out_cls[d] = p.cls[s];
        p.out_score[d] = p.score[s];
        for (int k = 0; k < 4; ++k) p.out_box[d * 4 + k] = p.box[s * 4 + k];
    }
}

bool ps_sizes_ok(int64_t N, int64_t F) { return N >= 0 && F >= 0 && N < (1ll << 31) && F < (1ll << 31); }

}  // namespace

extern "C" {

// Stage 1 for one box set.  Replaces filter_boxes (io/box_filtering.py:36-41) with the thresholds of evaluate_list (evaluation.py:24-35;
// apply_filters = 0: every row is kept, as apply_bbox_filters=False skips the filter) and, with `first` given, np.unique of the filtered
// timestamps per file (metrics/coco_eval.py:48).  keep / first: int32 [N] flags; first may be NULL (detections).
int eas_psee_mark(const int64_t* t, const float* box, int64_t N, const int64_t* file_offsets, int64_t F, int64_t skip_ts, int min_diag,
                  int min_side, int apply_filters, int32_t* keep, int32_t* first, eas_stream_t stream) {
    if (!ps_sizes_ok(N, F) || min_diag < 0 || min_side < 0 || min_diag > 32767) return EAS_ERR_UNSUPPORTED;
    if (N == 0) return EAS_OK;
    if (!t || !box || !keep || (first && (!file_offsets || F < 1))) return EAS_ERR_INVALID_ARG;
    PsFilter f;
    f.skip_ts = skip_ts; f.diag2 = (float)(min_diag * min_diag); f.side = (float)min_side; f.apply = apply_filters ? 1 : 0;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(ps_mark_kernel, dim3(eas_grid_1d(N)), dim3(EAS_BLOCK), 0, eas_s(stream), (const long long*)t, box, (long long)N,
               (const long long*)file_offsets, (long long)F, f, keep, first);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// Stage 2.  Replaces _match_times (metrics/coco_eval.py:58-91).  gt_img_scan: inclusive scan of gt_first; dt_keep_scan: exclusive scan of
// the detections' keep flags with the total at [Nd].  Per image (the first I entries, I = gt_img_scan[Ng-1]): image_file, image_t, win_lo =
// position of its first detection among the kept detections, win_cnt = their number (0 behind the last image); pair_count [Ng][K] = kept
// ground truths per (image, class).
int eas_psee_windows(const int64_t* gt_t, const int32_t* gt_cls, const int32_t* gt_keep, const int32_t* gt_first, const int64_t* gt_img_scan,
                     int64_t Ng, const int64_t* gt_file_offsets, const int64_t* dt_t, const int64_t* dt_file_offsets,
                     const int64_t* dt_keep_scan, int64_t Nd, int64_t F, int64_t time_tol, int K, int32_t* image_file, int64_t* image_t,
                     int64_t* win_lo, int64_t* win_cnt, int32_t* pair_count, eas_stream_t stream) {
    if (!ps_sizes_ok(Ng, F) || !ps_sizes_ok(Nd, F) || K < 1 || K > 1024 || time_tol < 0) return EAS_ERR_UNSUPPORTED;
    if (Ng == 0) return EAS_OK;
    if (F < 1 || !gt_t || !gt_cls || !gt_keep || !gt_first || !gt_img_scan || !gt_file_offsets || !dt_file_offsets || !dt_keep_scan ||
        (Nd > 0 && !dt_t) || !image_file || !image_t || !win_lo || !win_cnt || !pair_count)
        return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (hipMemsetAsync(win_cnt, 0, (size_t)Ng * sizeof(int64_t), st) != hipSuccess) return EAS_ERR_LAUNCH;
    if (hipMemsetAsync(pair_count, 0, (size_t)Ng * K * sizeof(int32_t), st) != hipSuccess) return EAS_ERR_LAUNCH;
    PsWindows p;
    p.gt_t = (const long long*)gt_t; p.gt_cls = gt_cls; p.gt_keep = gt_keep; p.gt_first = gt_first;
    p.gt_img_scan = (const long long*)gt_img_scan; p.gt_offsets = (const long long*)gt_file_offsets;
    p.dt_t = (const long long*)dt_t; p.dt_offsets = (const long long*)dt_file_offsets; p.dt_keep_scan = (const long long*)dt_keep_scan;
    p.Ng = Ng; p.Nd = Nd; p.F = F; p.tol = time_tol; p.K = K;
    p.image_file = image_file; p.image_t = (long long*)image_t; p.win_lo = (long long*)win_lo; p.win_cnt = (long long*)win_cnt;
    p.pair_count = pair_count;
    EAS_LAUNCH(ps_windows_kernel, dim3(eas_grid_1d(Ng)), dim3(EAS_BLOCK), 0, st, p);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// Stage 3.  Replaces the flattening of evaluate_detection (:52-53) and _to_coco_format (:128-179) as arrays: G ground-truth rows
// (gt_id = 1..G) and D detection rows, image-major, inside an image in file row order.  I, D, G are what the scans report
// (gt_img_scan[Ng-1], det_off[I], gt_keep_scan[Ng]); det_off: exclusive scan of win_cnt, at least I + 1 entries.
int eas_psee_expand(const int32_t* gt_keep, const int64_t* gt_keep_scan, const int64_t* gt_img_scan, const int32_t* gt_cls,
                    const float* gt_box, int64_t Ng, int64_t G, const int64_t* det_off, const int64_t* win_lo, int64_t I,
                    const int64_t* dt_keep_scan, const int32_t* dt_cls, const float* dt_box, const float* dt_score, int64_t Nd, int64_t D,
                    int32_t* out_gt_img, int32_t* out_gt_cls, float* out_gt_box, int64_t* out_gt_id, int32_t* out_det_img,
                    int32_t* out_det_cls, float* out_det_box, float* out_det_score, eas_stream_t stream) {
    if (!ps_sizes_ok(Ng, 0) || !ps_sizes_ok(Nd, 0) || G < 0 || G > Ng || I < 0 || I > G || D < 0 || D >= (1ll << 31)) return EAS_ERR_UNSUPPORTED;
    if (D > 0 && (I == 0 || Nd == 0)) return EAS_ERR_INVALID_ARG;
    if (G > 0 && (!gt_keep || !gt_keep_scan || !gt_img_scan || !gt_cls || !gt_box || !out_gt_img || !out_gt_cls || !out_gt_box || !out_gt_id))
        return EAS_ERR_INVALID_ARG;
    if (D > 0 && (!det_off || !win_lo || !dt_keep_scan || !dt_cls || !dt_box || !dt_score || !out_det_img || !out_det_cls || !out_det_box ||
                  !out_det_score))
        return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (G > 0) {
        EAS_LAUNCH(ps_expand_gt_kernel, dim3(eas_grid_1d(Ng)), dim3(EAS_BLOCK), 0, st, gt_keep, (const long long*)gt_keep_scan,
                   (const long long*)gt_img_scan, gt_cls, gt_box, (long long)Ng, (long long)G, out_gt_img, out_gt_cls, out_gt_box,
                   (long long*)out_gt_id);
        EAS_CHECK_LAUNCH();
    }
    if (D > 0) {
        PsExpandDet p;
        p.det_off = (const long long*)det_off; p.win_lo = (const long long*)win_lo; p.keep_scan = (const long long*)dt_keep_scan;
        p.cls = dt_cls; p.box = dt_box; p.score = dt_score;
        p.I = I; p.D = D; p.Nd = Nd;
        p.out_img = out_det_img; p.out_cls = out_det_cls; p.out_box = out_det_box; p.out_score = out_det_score;
        EAS_LAUNCH(ps_expand_det_kernel, dim3(eas_grid_1d(D)), dim3(EAS_BLOCK), 0, st, p);
        EAS_CHECK_LAUNCH();
    }
    return EAS_OK;
}

}  // extern "C"
