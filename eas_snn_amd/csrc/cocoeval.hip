// COCO-style bounding-box evaluation on the device: the evaluate -> accumulate sequence of COCOeval(gt, dt, 'bbox') as the reference's
// native module computes it (yolox/layers/cocoeval/cocoeval.cpp: EvaluateImages :140-197 with MatchDetectionsToGroundTruth :59-138,
// Accumulate :370-476 with BuildSortedDetectionList :221-271 and ComputePrecisionRecallCurve :282-369), driven the way
// yolox/layers/fast_coco_eval_api.py:62-117 drives it (IoU rows in descending-score order, cut at max(maxDets)).  iscrowd is always 0 in
// this project (getcocoGT, yolox/evaluators/event_evaluator.py:365-372): crowd handling is not built.
//
// Arithmetic: boxes (x, y, w, h) and scores arrive as float32 and are widened to double; area = w * h; the IoU in the order of pycocotools'
// bbIou (w = min(dx+dw, gx+gw) - max(dx, gx), w <= 0 -> 0, h likewise, i = w*h, u = dw*dh + gw*gh - i, i / u); -ffp-contract=off.
// Counting is integer (ballots, popcounts, integer atomics), precision = tp / (tp + fp) and recall = tp / npig are one double division each:
// the results are deterministic and equal to the reference's bit for bit.
//
// Calls, each one entry point, the two sorts between them are the caller's (64-bit keys, any stable ascending sort):
//   keys        det_key = pair << 32 | ~order(score), gt_key = pair, pair = image * K + category (I * K for an index outside the tables)
//   [sort 1]    stable, ascending by det_key / gt_key: a pair's detections in descending score, ties to the earlier one; its ground truths
//               in their own order
//   match       one wavefront per non-empty pair, lane = (area range a, IoU threshold t): per detection (in order, the first max_det) the
//               64 lanes compute its IoU row into LDS, then every lane walks the ground truths in ITS area range's order (non-ignored
//               first, stable) with the set of taken ground truths as a 64-bit register mask; the lanes' results are two ballots =
//               the detection's matched / ignored bit masks (bit a * T + t).  Also the rank inside the pair, the key of sort 2
//               (category << 32 | ~order(score)), and the non-ignored ground truths per (category, area range) by integer atomics.
//               "Matched" means the matched ground truth's id is not 0 (cocoeval.cpp:322-323): a match to id 0 takes that ground truth and
//               counts as unmatched.
//   [sort 2]    stable, ascending by that key: per category (score descending, image ascending, rank ascending) -- the order of sort 1
//               breaks the ties as the reference's stable sort over images in order does
//   accumulate  a gather of (matched, ignored, rank) into the order of sort 2, then one block per (category, area range, max-dets entry)
//               walks the category's list in chunks of 1024 (the block) with a carry, ALL IoU thresholds at once (one read of the masks for the T
//               curves): ballot prefix counts give tp / fp at every position; precision[r] = the largest precision at any position whose
//               recall is >= rec_thr[r] (= the reference's suffix-maximum envelope followed by lower_bound, recall being non-decreasing),
//               kept as an LDS maximum on the bit pattern of the non-negative doubles per (t, last r with rec_thr[r] <= recall) and a
//               suffix maximum over r at the end.  Only true-positive positions are entered: between two of them recall stays and
//               precision can only fall (a correctly rounded quotient is monotone in its divisor), and before the first one it is 0.
//
// Limits (eas_cocoeval_supported): ground truths per (image, category) <= 64; T <= 16, A <= 8, A * T <= 64, R <= 128, M <= 8;
// I * K <= 2^24 pairs; K * A * M <= 2^20; D, G < 2^31.  rec_thr ascending.  The per-threshold ``scores`` array of pycocotools is not produced.
#include "eas_common.h"

namespace {

constexpr int kMaxGt = 64;
constexpr int kMaxT = 16;
constexpr int kMaxA = 8;
constexpr int kMaxR = 128;
constexpr int kMaxM = 8;
constexpr int kAccThreads = 1024;
constexpr int kAccWaves = kAccThreads / EAS_WAVE;

__device__ __forceinline__ unsigned ce_order_bits(float f) {
    const unsigned u = __float_as_uint(f + 0.0f);          // -0 -> +0: the reference compares values
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(EAS_BLOCK) void ce_keys_kernel(const int* __restrict__ det_img, const int* __restrict__ det_cls,
                                                            const float* __restrict__ det_score, long long D, const int* __restrict__ gt_img,
                                                            const int* __restrict__ gt_cls, long long G, int I, int K,
                                                            long long* __restrict__ det_key, long long* __restrict__ gt_key) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long none = (long long)I * K;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < D + G; j += stride) {
        if (j < D) {
            const int i = det_img[j], c = det_cls[j];
            const long long pair = (i >= 0 && i < I && c >= 0 && c < K) ? (long long)i * K + c : none;
            det_key[j] = (pair << 32) | (long long)(unsigned)(~ce_order_bits(det_score[j]));
        } else {
            const long long g = j - D;
            const int i = gt_img[g], c = gt_cls[g];
            gt_key[g] = (i >= 0 && i < I && c >= 0 && c < K) ? (long long)i * K + c : none;
        }
    }
}

// first index in [0, n) whose key is >= v
__device__ __forceinline__ long long ce_lower_bound(const long long* __restrict__ keys, long long n, long long v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct CeMatch {
    const long long* det_key;      // [D] sorted
    const long long* det_order;    // [D] sorted position -> input index
    const float* det_box;          // [D][4] input order
    const long long* gt_key;       // [G] sorted
    const long long* gt_order;     // [G]
    const float* gt_box;           // [G][4] input order
    const long long* gt_id;        // [G] input order
    const double* iou_thr;         // [T]
    const double* area_rng;        // [A][2]
    long long D, G;
    int I, K, T, A, max_det;
    int* rank;                             // [D] by sorted position
    unsigned long long* matched;           // [D]
    unsigned long long* ignored;           // [D]
    long long* key2;                       // [D]
    int* npig;                             // [K][A]
};

__global__ __launch_bounds__(EAS_WAVE) void ce_match_kernel(CeMatch p) {
    __shared__ double iou_row[kMaxGt];
    __shared__ unsigned char gorder[kMaxA][kMaxGt];
    __shared__ unsigned char gnz[kMaxGt];
    const int lane = threadIdx.x;
    const long long pair = blockIdx.x;
    const long long d0 = ce_lower_bound(p.det_key, p.D, pair << 32);
    if (pair == (long long)p.I * p.K) {
        // detections whose image or category is outside the tables: never read again, sorted behind every category
        for (long long j = d0 + lane; j < p.D; j += EAS_WAVE) {
            p.rank[j] = 0x7fffffff;
            p.matched[j] = 0;
            p.ignored[j] = 0;
            p.key2[j] = (long long)p.K << 32;
        }
        return;
    }
    const long long d1 = ce_lower_bound(p.det_key, p.D, (pair + 1) << 32);
    const long long g0 = ce_lower_bound(p.gt_key, p.G, pair), g1 = ce_lower_bound(p.gt_key, p.G, pair + 1);
    const long long nd_all = d1 - d0;
    const int ng = (int)((g1 - g0) < kMaxGt ? (g1 - g0) : kMaxGt);       // (the host declines inputs with more)
    if (nd_all == 0 && ng == 0) return;
    const int cls = (int)(pair % p.K);
    const int T = p.T, A = p.A;
    const bool active = lane < A * T;
    const int a = active ? lane / T : 0, t = active ? lane % T : 0;
    const double lo_a = p.area_rng[2 * a], hi_a = p.area_rng[2 * a + 1];
    const double thr = p.iou_thr[t];

    // ---- this lane's ground truth; per area range the stable order "non-ignored first"
    double gx = 0, gy = 0, gw = 0, gh = 0;
    if (lane < ng) {
        const long long src = p.gt_order[g0 + lane];
        const float* b = p.gt_box + src * 4;
        gx = b[0]; gy = b[1]; gw = b[2]; gh = b[3];
        gnz[lane] = p.gt_id[src] != 0;
    }
    const double garea = gw * gh;
    const unsigned long long have = ng == 64 ? ~0ull : ((1ull << ng) - 1), below = (1ull << lane) - 1;
    int nvalid = 0;
    for (int aa = 0; aa < A; ++aa) {
        const double lo = p.area_rng[2 * aa], hi = p.area_rng[2 * aa + 1];
        const bool ign = lane < ng && (garea < lo || garea > hi);
        const unsigned long long ib = __ballot(ign), vb = ~ib & have;
        const int nv = __popcll(vb);
        if (lane < ng) gorder[aa][ign ? nv + __popcll(ib & below) : __popcll(vb & below)] = (unsigned char)lane;
        if (aa == a) nvalid = nv;
        if (lane == 0 && nv) atomicAdd(&p.npig[cls * A + aa], nv);
    }
    __syncthreads();

    // ---- the greedy walk, detection by detection
    const int nd = (int)(nd_all < p.max_det ? nd_all : p.max_det);
    unsigned long long taken = 0;
    for (int r = 0; r < nd; ++r) {
        const float* b = p.det_box + p.det_order[d0 + r] * 4;
        const double dx = b[0], dy = b[1], dw = b[2], dh = b[3];
        if (lane < ng) {
            double iou = 0.0;
            const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
            if (w > 0) {
                const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
                if (h > 0) {
                    const double i = w * h;
                    const double u = dw * dh + garea - i;
                    iou = i / u;
                }
            }
            iou_row[lane] = iou;
        }
        __syncthreads();
        bool is_matched = false, is_ignored = false;
        if (active) {
            double best = fmin(thr, 1 - 1e-10);
            int match = -1;
            for (int g = 0; g < ng; ++g) {
                if ((taken >> g) & 1ull) continue;
                if (match >= 0 && match < nvalid && g >= nvalid) break;
                const double v = iou_row[gorder[a][g]];
                if (v >= best) { best = v; match = g; }
            }
            if (match >= 0) {
                is_ignored = match >= nvalid;
                is_matched = gnz[gorder[a][match]] != 0;
                taken |= 1ull << match;
            }
            const double darea = dw * dh;
            is_ignored = is_ignored || (!is_matched && (darea < lo_a || darea > hi_a));
        }
        const unsigned long long mb = __ballot(is_matched), ib = __ballot(is_ignored);
        if (lane == 0) {
            p.matched[d0 + r] = mb;
            p.ignored[d0 + r] = ib;
        }
        __syncthreads();
    }
    for (long long j = lane; j < nd_all; j += EAS_WAVE) {
        p.rank[d0 + j] = (int)(j < 0x7fffffff ? j : 0x7fffffff);
        p.key2[d0 + j] = ((long long)cls << 32) | (p.det_key[d0 + j] & 0xffffffffll);
        if (j >= nd) {
            p.matched[d0 + j] = 0;
            p.ignored[d0 + j] = 0;
        }
    }
}

__global__ __launch_bounds__(EAS_BLOCK) void ce_gather_kernel(const long long* __restrict__ order2, const int* __restrict__ rank,
                                                              const unsigned long long* __restrict__ matched,
                                                              const unsigned long long* __restrict__ ignored, long long D,
                                                              unsigned long long* __restrict__ s_matched,
                                                              unsigned long long* __restrict__ s_ignored, int* __restrict__ s_rank) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < D; j += stride) {
        const long long src = order2[j];
        s_matched[j] = matched[src];
        s_ignored[j] = ignored[src];
        s_rank[j] = rank[src];
    }
}

struct CeAcc {
    const long long* key2;                 // [D] sorted
    const unsigned long long* s_matched;   // [D] in the order of sort 2
    const unsigned long long* s_ignored;
    const int* s_rank;
    const int* npig;                       // [K][A]
    const double* rec_thr;                 // [R]
    const int* max_dets;                   // [M]
    long long D;
    int K, T, R, A, M;
    double* precision;                     // [T][R][K][A][M]
    double* recall;                        // [T][K][A][M]
};

__global__ __launch_bounds__(kAccThreads) void ce_accumulate_kernel(CeAcc p) {
    __shared__ unsigned long long bucket[kMaxT * kMaxR];
    __shared__ double rthr[kMaxR];
    __shared__ int wtot[2][kMaxT][kAccWaves];
    const int tid = threadIdx.x, lane = tid & (EAS_WAVE - 1), wave = tid / EAS_WAVE;
    const int T = p.T, R = p.R, A = p.A, M = p.M, K = p.K;
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % A, c = blockIdx.x / (M * A);
    const int npig = p.npig[c * A + a];
    const size_t cam = ((size_t)c * A + a) * M + m, KAM = (size_t)K * A * M;
    if (npig == 0) {
        // no ground truth counts for this (category, area range): the reference leaves -1 (cocoeval.cpp:432-434)
        for (int j = tid; j < T * R; j += kAccThreads) p.precision[(size_t)j * KAM + cam] = -1.0;
        if (tid < T) p.recall[(size_t)tid * KAM + cam] = -1.0;
        return;
    }
    for (int j = tid; j < T * R; j += kAccThreads) bucket[j] = 0;
    for (int j = tid; j < R; j += kAccThreads) rthr[j] = p.rec_thr[j];
    const long long n0 = ce_lower_bound(p.key2, p.D, (long long)c << 32), n1 = ce_lower_bound(p.key2, p.D, (long long)(c + 1) << 32);
    const int md = p.max_dets[m];
    const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
    int carry_tp[kMaxT], carry_fp[kMaxT];
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) carry_tp[t] = carry_fp[t] = 0;
    __syncthreads();
    for (long long base = n0; base < n1; base += kAccThreads) {
        const long long j = base + tid;
        const bool valid = j < n1 && p.s_rank[j] < md;
        const unsigned long long mm = valid ? p.s_matched[j] : 0ull, im = valid ? p.s_ignored[j] : ~0ull;
        unsigned pre[kMaxT];       // inclusive prefix counts inside the wave: tp | fp << 16
        unsigned is_tp = 0;
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) {
            pre[t] = 0;
            if (t < T) {
                const int bit = a * T + t;
                const bool counted = !((im >> bit) & 1ull);
                const bool tp = counted && ((mm >> bit) & 1ull), fp = counted && !((mm >> bit) & 1ull);
                const unsigned long long bt = __ballot(tp), bf = __ballot(fp);
                pre[t] = (unsigned)__popcll(bt & le) | ((unsigned)__popcll(bf & le) << 16);
                is_tp |= (tp ? 1u : 0u) << t;
                if (lane == 0) {
                    wtot[0][t][wave] = __popcll(bt);
                    wtot[1][t][wave] = __popcll(bf);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) {
            if (t < T) {
                int before_tp = 0, before_fp = 0, all_tp = 0, all_fp = 0;
#pragma unroll
                for (int w = 0; w < kAccWaves; ++w) {
                    const int vt = wtot[0][t][w], vf = wtot[1][t][w];
                    all_tp += vt; all_fp += vf;
                    if (w < wave) { before_tp += vt; before_fp += vf; }
                }
                if ((is_tp >> t) & 1u) {
                    const long long tp = (long long)carry_tp[t] + before_tp + (int)(pre[t] & 0xffffu);
                    const long long fp = (long long)carry_fp[t] + before_fp + (int)(pre[t] >> 16);
                    const double prec = (double)tp / (double)(tp + fp);
                    const double rec = (double)tp / (double)npig;
                    int lo = 0, hi = R;                      // number of recall thresholds <= rec
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (rthr[mid] <= rec) lo = mid + 1; else hi = mid;
                    }
                    if (lo > 0) atomicMax(&bucket[t * R + lo - 1], (unsigned long long)__double_as_longlong(prec));
                }
                carry_tp[t] += all_tp;
                carry_fp[t] += all_fp;
            }
        }
        __syncthreads();
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) {
        if (t < T && tid == t) {
            unsigned long long run = 0;
            for (int r = R - 1; r >= 0; --r) {
                const unsigned long long v = bucket[t * R + r];
                run = v > run ? v : run;
                p.precision[((size_t)t * R + r) * KAM + cam] = __longlong_as_double((long long)run);
            }
            p.recall[(size_t)t * KAM + cam] = (double)carry_tp[t] / (double)npig;
        }
    }
}

size_t ce_align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool ce_dims_ok(int64_t D, int64_t G, int64_t I, int K, int T, int R, int A, int M) {
    return D >= 0 && G >= 0 && I >= 0 && D < (1ll << 31) && G < (1ll << 31) && K >= 1 && T >= 1 && R >= 1 && A >= 1 && M >= 1 && T <= kMaxT &&
           A <= kMaxA && A * T <= EAS_WAVE && R <= kMaxR && M <= kMaxM && I * (int64_t)K <= (1ll << 24) && (int64_t)K * A * M <= (1ll << 20);
}

}  // namespace

extern "C" {

// 1 when the evaluation below handles this problem, else 0 (the caller keeps its other route): D detections, G ground truths, I images,
// K categories, T IoU thresholds, R recall thresholds, A area ranges, M max-dets entries, at most max_gt_per_pair ground truths in one
// (image, category).  Replaces nothing in the reference (its module has no limits); the limits are the header comment's.
int eas_cocoeval_supported(int64_t D, int64_t G, int64_t I, int K, int T, int R, int A, int M, int64_t max_gt_per_pair) {
    return ce_dims_ok(D, G, I, K, T, R, A, M) && max_gt_per_pair >= 0 && max_gt_per_pair <= kMaxGt ? 1 : 0;
}

// bytes of the workspace of eas_cocoeval_accumulate
int64_t eas_cocoeval_workspace_bytes(int64_t D) {
    if (D < 0) return 0;
    return (int64_t)(2 * ce_align256((size_t)D * 8) + ce_align256((size_t)D * 4) + 256);
}

// Sort keys of the (image, category) lists.  Replaces the grouping of COCOeval._prepare into _gts / _dts[imgId, catId] and the key of
// SortInstancesByDetectionScore (cocoeval.cpp:16-28; pycocotools computeIoU's argsort of -score).
int eas_cocoeval_keys(const int32_t* det_img, const int32_t* det_cls, const float* det_score, int64_t D, const int32_t* gt_img,
                      const int32_t* gt_cls, int64_t G, int64_t I, int K, int64_t* det_key, int64_t* gt_key, eas_stream_t stream) {
    if (!ce_dims_ok(D, G, I, K, 1, 1, 1, 1)) return EAS_ERR_UNSUPPORTED;
    if ((D > 0 && (!det_img || !det_cls || !det_score || !det_key)) || (G > 0 && (!gt_img || !gt_cls || !gt_key))) return EAS_ERR_INVALID_ARG;
    if (D + G == 0) return EAS_OK;
    EAS_CLEAR_ERR();
    EAS_LAUNCH(ce_keys_kernel, dim3(eas_grid_1d(D + G)), dim3(EAS_BLOCK), 0, eas_s(stream), det_img, det_cls, det_score, (long long)D, gt_img,
               gt_cls, (long long)G, (int)I, K, (long long*)det_key, (long long*)gt_key);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// Stage 1.  Replaces EvaluateImages (cocoeval.cpp:140-197): SortInstancesByDetectionScore + the cut at max_det (:16-28, :168-172; the order
// itself is sort 1), SortInstancesByIgnore (:32-55), MatchDetectionsToGroundTruth (:59-138), the IoU matrices of pycocotools' computeIoU /
// bbIou, and the count of non-ignored ground truths of BuildSortedDetectionList (:251-255).  det_key / gt_key sorted ascending (stable),
// det_order / gt_order the sorted position's index into the input arrays; outputs by sorted position: rank inside the pair, matched /
// ignored masks (bit a * T + t; written for the first max_det of a pair, 0 behind), key2 for sort 2; npig [K][A].
int eas_cocoeval_match(const int64_t* det_key, const int64_t* det_order, const float* det_box, int64_t D, const int64_t* gt_key,
                       const int64_t* gt_order, const float* gt_box, const int64_t* gt_id, int64_t G, int64_t I, int K, const double* iou_thr,
                       int T, const double* area_rng, int A, int max_det, int64_t max_gt_per_pair, int32_t* rank, uint64_t* matched,
                       uint64_t* ignored, int64_t* key2, int32_t* npig, eas_stream_t stream) {
    if (!eas_cocoeval_supported(D, G, I, K, T, 1, A, 1, max_gt_per_pair)) return EAS_ERR_UNSUPPORTED;
    if (!iou_thr || !area_rng || !npig || max_det < 0) return EAS_ERR_INVALID_ARG;
    if ((D > 0 && (!det_key || !det_order || !det_box || !rank || !matched || !ignored || !key2)) ||
        (G > 0 && (!gt_key || !gt_order || !gt_box || !gt_id)))
        return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    if (hipMemsetAsync(npig, 0, (size_t)K * A * sizeof(int), st) != hipSuccess) return EAS_ERR_LAUNCH;
    if (D + G == 0) return EAS_OK;
    CeMatch p;
    p.det_key = (const long long*)det_key; p.det_order = (const long long*)det_order; p.det_box = det_box;
    p.gt_key = (const long long*)gt_key; p.gt_order = (const long long*)gt_order; p.gt_box = gt_box; p.gt_id = (const long long*)gt_id;
    p.iou_thr = iou_thr; p.area_rng = area_rng;
    p.D = D; p.G = G; p.I = (int)I; p.K = K; p.T = T; p.A = A; p.max_det = max_det;
    p.rank = rank; p.matched = (unsigned long long*)matched; p.ignored = (unsigned long long*)ignored; p.key2 = (long long*)key2; p.npig = npig;
    EAS_LAUNCH(ce_match_kernel, dim3((unsigned)(I * K + 1)), dim3(EAS_WAVE), 0, st, p);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// Stage 2.  Replaces Accumulate (cocoeval.cpp:370-476): BuildSortedDetectionList (:221-271; the order itself is sort 2, order2 = the sorted
// position's index into the arrays of eas_cocoeval_match) and ComputePrecisionRecallCurve (:282-369).  precision [T][R][K][A][M] and recall
// [T][K][A][M] are written completely (-1 where no ground truth counts).  max_dets: DEVICE int32 [M].
// workspace: eas_cocoeval_workspace_bytes(D) bytes.
int eas_cocoeval_accumulate(const int64_t* key2, const int64_t* order2, const int32_t* rank, const uint64_t* matched, const uint64_t* ignored,
                            int64_t D, const int32_t* npig, int K, int T, const double* rec_thr, int R, int A, const int32_t* max_dets, int M,
                            double* precision, double* recall, void* workspace, eas_stream_t stream) {
    if (!ce_dims_ok(D, 0, 0, K, T, R, A, M)) return EAS_ERR_UNSUPPORTED;
    if (!npig || !rec_thr || !max_dets || !precision || !recall) return EAS_ERR_INVALID_ARG;
    if (D > 0 && (!key2 || !order2 || !rank || !matched || !ignored || !workspace)) return EAS_ERR_INVALID_ARG;
    hipStream_t st = eas_s(stream);
    EAS_CLEAR_ERR();
    CeAcc p;
    char* w = (char*)workspace;
    p.s_matched = (unsigned long long*)w; w += ce_align256((size_t)D * 8);
    p.s_ignored = (unsigned long long*)w; w += ce_align256((size_t)D * 8);
    p.s_rank = (int*)w;
    if (D > 0) {
        EAS_LAUNCH(ce_gather_kernel, dim3(eas_grid_1d(D)), dim3(EAS_BLOCK), 0, st, (const long long*)order2, rank,
                   (const unsigned long long*)matched, (const unsigned long long*)ignored, (long long)D, (unsigned long long*)p.s_matched,
                   (unsigned long long*)p.s_ignored, (int*)p.s_rank);
        EAS_CHECK_LAUNCH();
    }
    p.key2 = (const long long*)key2; p.npig = npig; p.rec_thr = rec_thr; p.max_dets = max_dets;
    p.D = D; p.K = K; p.T = T; p.R = R; p.A = A; p.M = M;
    p.precision = precision; p.recall = recall;
    EAS_LAUNCH(ce_accumulate_kernel, dim3((unsigned)(K * A * M)), dim3(kAccThreads), 0, st, p);
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

}  // extern "C"
