// Grouped (multi-problem) launches of the dense 3x3 convolution: ONE grid, a descriptor table of {geometry, packed weights, in / out
// pointers} in the kernel arguments, blockIdx.x -> (problem, pixel tile).  The three pyramid levels of the detection head run the same
// layers on 32x40, 16x20 and 8x10 maps and are independent until the loss (yolox/models/yolo_head.py:149-200, the
// `for k, (cls_conv, reg_conv, stride_this_level, x)` loop): as launches of their own the two small levels leave most of the 256 CUs
// without a block (64 images of 8x10 with 128 channels are 64 four-wave blocks) and still pay a kernel's whole prologue / epilogue; in the
// grid of the large level they are a few more blocks of the same kernel.  The tiles are conv_mfma_body.h's (same staging, same MFMA
// order: results bit-identical to eas_conv_fwd per problem); a block first looks its problem up, then runs the body instantiated for the
// problem's staging width (16-byte units where the rows are a multiple of 4 pixels, 8-byte units for the 10-pixel rows).
// Forward and -- with weights packed transposed + flipped (mode 1) and grad_y as x -- the stride-1 input gradient.
#include "conv_mfma_body.h"

namespace {

constexpr int kMaxGroup = 8;

template <typename G>
struct ConvGroupArgsT {
    G g[kMaxGroup];
    const float* x[kMaxGroup];
    const bf16x8* wp[kMaxGroup];
    const float* bias[kMaxGroup];
    float* y[kMaxGroup];
    int first[kMaxGroup + 1];      // problem p owns pixel tiles [first[p], first[p + 1]) of grid.x
    int vec2[kMaxGroup];           // 1: the problem's rows are staged in 2-pixel units (Wi % 4 != 0)
    int n;
};
typedef ConvGroupArgsT<ConvGeomCore> ConvGroupArgs;

// LM = 0: the plain epilogue (y, bias, BatchNorm partial sums); LM = 3: BatchNorm (running statistics) + activation on the accumulators
// (grouped eas_conv_bn_act_eval: the eval-mode head), G = the geometry type that carries what the epilogue reads
template <int XT, int WN, int WVM, int WVN, int NIT, int LM = 0, typename G = ConvGeomCore>
__global__ __launch_bounds__(64 * WVM * WVN, 2) void conv3x3_group_kernel(const ConvGroupArgsT<G> a) {
    extern __shared__ __align__(16) unsigned char smem[];
    int p = 0;
    for (int i = 1; i < a.n; ++i)
        if ((int)blockIdx.x >= a.first[i]) p = i;
    p = __builtin_amdgcn_readfirstlane(p);
    const int bx = (int)blockIdx.x - a.first[p], gx = a.first[p + 1] - a.first[p];
    if ((int)blockIdx.y * WVM >= a.g[p].MT) return;        // grid.y covers the widest problem: no channels left for this block (whole block exits)
    if (a.vec2[p])
        conv_tile_body<9, 1, XT, 1, WN, WVM, WVN, 16, 2, NIT, false, LM, G>(a.x[p], a.wp[p], a.bias[p], a.y[p], nullptr, a.g[p], 0, smem, bx,
                                                                            (int)blockIdx.y, gx);
    else
        conv_tile_body<9, 1, XT, 1, WN, WVM, WVN, 16, 4, NIT, false, LM, G>(a.x[p], a.wp[p], a.bias[p], a.y[p], nullptr, a.g[p], 0, smem, bx,
                                                                            (int)blockIdx.y, gx);
}

template <int XT, int WN, int WVM, int WVN, int NIT, int LM, typename G>
int launch_group3(ConvGroupArgsT<G>& a, int grid_y, size_t lds, hipStream_t st) {
    auto kern = conv3x3_group_kernel<XT, WN, WVM, WVN, NIT, LM, G>;
    static bool attr_set = false;
    for (int p = 0; p < a.n; ++p)
        if (const int rc = conv_launch_prep((const void*)kern, attr_set, a.g[p], a.vec2[p] ? 2 : 4, 16)) return rc;
    EAS_LAUNCH(kern, dim3(a.first[a.n], grid_y), dim3(64 * WVM * WVN), lds, st, a);
    return EAS_OK;
}

struct GCand { int wvm, wvn, wn, nit; };
static const GCand kCands[4] = {{4, 1, 5, 2}, {2, 2, 5, 2}, {4, 1, 3, 2}, {2, 2, 3, 2}};

template <int XT, int LM, typename G>
int launch_cand3(int i, ConvGroupArgsT<G>& a, int grid_y, size_t lds, hipStream_t st) {
    switch (i) {
        case 0: return launch_group3<XT, 5, 4, 1, 2, LM, G>(a, grid_y, lds, st);
        case 1: return launch_group3<XT, 5, 2, 2, 2, LM, G>(a, grid_y, lds, st);
        case 2: return launch_group3<XT, 3, 4, 1, 2, LM, G>(a, grid_y, lds, st);
        default: return launch_group3<XT, 3, 2, 2, 2, LM, G>(a, grid_y, lds, st);
    }
}

// One tile shape for all problems of the group: every problem gets the candidate's largest fitting whole-row tile (conv_mfma_body.h), and
// the round cost of dispatch_tile is paid for the SUM of the problems' blocks in fractional rounds (the small levels fill the last round
// of the large one).
template <int XT, typename G>
int plan_group3(const EasConvProblem* pr, int n, ConvGroupArgsT<G>& a, int& best, int& grid_y, size_t& lds, int* nb_out) {
    const GCand* cands = kCands;
    static const int force = eas_dev_env("EAS_GROUP3_TILE") ? atoi(eas_dev_env("EAS_GROUP3_TILE")) : -1;      // development: force a candidate
    best = -1;
    double best_cost = 0.0;
    ConvGroupArgsT<G> best_a = a;
    for (int i = 0; i < 4; ++i) {
        if (force >= 0 && i != force) continue;
        const GCand& c = cands[i];
        const int threads = 64 * c.wvm * c.wvn;
        int cout_min = 1 << 30;
        for (int p = 0; p < n; ++p) cout_min = pr[p].Cout < cout_min ? pr[p].Cout : cout_min;
        if ((c.wvm - 1) * 32 >= cout_min) continue;          // every wave row has channels to compute in every problem
        ConvGroupArgsT<G> t = a;
        bool ok = true;
        double load = 0.0;
        size_t lds_max = 0;
        int gy = 1, blocks_x = 0;
        for (int p = 0; p < n && ok; ++p) {
            G& g = t.g[p];
            conv3_base_geom(g, pr[p].NI, pr[p].Cin, pr[p].Cout, pr[p].Hi, pr[p].Wi, 1);
            const int vec = pr[p].Wi % 4 == 0 ? 4 : 2;
            t.vec2[p] = vec == 2;
            const size_t l = conv_tile_shrink(g, 32 * c.wn * c.wvn, 1, g.KSTEPS == 1 ? 1 : 2, 16, XT, vec, c.nit * threads);
            ok = l != 0;
            if (!ok) break;
            lds_max = l > lds_max ? l : lds_max;
            const dim3 gp = conv_tile_grid(g, c.wvm);
            t.first[p] = blocks_x;
            blocks_x += gp.x;
            gy = (int)gp.y > gy ? (int)gp.y : gy;
            load += (double)gp.x * gp.y;
        }
        if (!ok) continue;
        t.first[n] = blocks_x;
        const int bpc = conv_blocks_per_cu(threads, lds_max);
        const double round_cost = conv_round_factor(threads, bpc, load) * conv_block_time(c.wn, 5.0, XT == 1 ? 96.0 : 192.0, conv_step_lat());
        double rounds = load / (256.0 * bpc);
        if (rounds < 1.0) rounds = 1.0;
        const double cost = rounds * round_cost;
        if (best < 0 || cost < best_cost - 1e-9) {
            best = i; best_cost = cost; best_a = t; grid_y = gy; lds = lds_max;
        }
    }
    if (best < 0) return EAS_ERR_UNSUPPORTED;
    a = best_a;
    const GCand& c = cands[best];
    const size_t stats_lds = (size_t)c.wvm * c.wvn * (EAS_STATS_SCRATCH * sizeof(float) + 64 * sizeof(double));
    bool any_stats = false;
    for (int p = 0; p < n; ++p) {
        G& g = a.g[p];
        const int gxp = a.first[p + 1] - a.first[p];
        conv_plan_note("group", best, c.wvm, c.wvn, c.wn, a.vec2[p] ? 2 : 4, g, dim3(gxp, grid_y, a.first[n]), lds, p);
        if (nb_out) nb_out[p] = gxp;
        g.stats = pr[p].stats;
        g.stats_nb = gxp;
        any_stats = any_stats || pr[p].stats;
        a.x[p] = (const float*)pr[p].x; a.wp[p] = (const bf16x8*)pr[p].packed_w; a.bias[p] = pr[p].bias; a.y[p] = pr[p].y;
    }
    if (any_stats && lds < stats_lds) lds = stats_lds;
    a.n = n;
    return EAS_OK;
}

template <int XT>
int group3(const EasConvProblem* pr, int n, hipStream_t st, int* nb_out, bool query) {
    ConvGroupArgs a{};
    int best = -1, grid_y = 1;
    size_t lds = 0;
    const int rc = plan_group3<XT, ConvGeomCore>(pr, n, a, best, grid_y, lds, nb_out);
    if (rc != EAS_OK || query) return rc;
    return launch_cand3<XT, 0, ConvGeomCore>(best, a, grid_y, lds, st);
}

// grouped eas_conv_bn_act_eval, 3x3: the same plan, every problem's BatchNorm / activation descriptor in its geometry
int group3_bna(const EasConvProblem* pr, const EasBnActEpiDev* bna, int n, hipStream_t st) {
    ConvGroupArgsT<ConvGeomBna> a{};
    int best = -1, grid_y = 1;
    size_t lds = 0;
    const int rc = plan_group3<3, ConvGeomBna>(pr, n, a, best, grid_y, lds, nullptr);
    if (rc != EAS_OK) return rc;
    for (int p = 0; p < n; ++p) a.g[p].bna = bna[p];
    return launch_cand3<3, 3, ConvGeomBna>(best, a, grid_y, lds, st);
}

}  // namespace

int eas_conv1x1_group(const EasConvProblem* pr, int n, int x_terms, hipStream_t st, int* nb_out, bool query, const void* bna = nullptr);

static int conv_group_impl(const EasConvProblem* pr, int n, int ksize, int x_terms, eas_stream_t stream, int* nb_out, bool query) {
    if (!pr || n < 1) return EAS_ERR_INVALID_ARG;
    if (x_terms != 3 || (ksize != 1 && ksize != 3)) return EAS_ERR_UNSUPPORTED;      // real-valued fp32 inputs (the ANN neck / head and every input gradient)
    for (int p = 0; p < n; ++p) {
        const EasConvProblem& q = pr[p];
        if (q.NI <= 0 || q.Cin <= 0 || q.Cout <= 0 || q.Hi <= 0 || q.Wi <= 0) return EAS_ERR_INVALID_ARG;
        if (!query && (!q.x || !q.packed_w || !q.y)) return EAS_ERR_INVALID_ARG;
        if (q.stats && q.bias) return EAS_ERR_INVALID_ARG;
        if (ksize == 3 && (q.Cin % 8 != 0 || q.Wi % 2 != 0 || q.accumulate)) return EAS_ERR_UNSUPPORTED;
    }
    EAS_CLEAR_ERR();
    int rc;
    if (ksize == 1) rc = eas_conv1x1_group(pr, n, x_terms, eas_s(stream), nb_out, query);
    else if (n > kMaxGroup) rc = EAS_ERR_UNSUPPORTED;
    else rc = group3<3>(pr, n, eas_s(stream), nb_out, query);
    if (rc != EAS_OK || query) return rc;
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

extern "C" {

// include/eas_hip.h: the tile plan of a group without launching anything -- nb_out[p] = statistics partials per channel problem p's
// blocks write (what EasConvProblem.stats must hold: Cout * nb * 2 doubles); EAS_ERR_UNSUPPORTED: run the problems one by one
int eas_conv_fwd_group_plan(const EasConvProblem* problems, int n, int ksize, int x_terms, int* nb_out) {
    return conv_group_impl(problems, n, ksize, x_terms, nullptr, nb_out, true);
}

// include/eas_hip.h: the tile of a grouped 3x3 launch, out[p] = problem p's part of the plan as plan_group3 left it at its exit
int eas_conv_fwd_group_tile_plan(const EasConvProblem* problems, int n, int ksize, int x_terms, EasConvPlan* out) {
    if (!out) return EAS_ERR_INVALID_ARG;
    if (ksize == 1) return EAS_ERR_UNSUPPORTED;          // (the 1x1 family: conv1x1_mfma.hip)
    const int rc = conv_group_impl(problems, n, ksize, x_terms, nullptr, nullptr, true);
    for (int p = 0; rc == EAS_OK && p < n; ++p) out[p] = tl_conv_plan[p];
    return rc;
}

int eas_conv_fwd_group(const EasConvProblem* problems, int n, int ksize, int x_terms, eas_stream_t stream) {
    return conv_group_impl(problems, n, ksize, x_terms, stream, nullptr, false);
}

// include/eas_hip.h: eas_conv_bn_act_eval for several layers in one launch (the eval-mode head: the three pyramid levels of a stage)
int eas_conv_bn_act_eval_group(const EasConvBnActEval* ds, int n, eas_stream_t stream) {
    if (!ds || n < 1) return EAS_ERR_INVALID_ARG;
    if (n > kMaxGroup) return EAS_ERR_UNSUPPORTED;
    EasConvProblem pr[kMaxGroup] = {};
    EasBnActEpiDev bna[kMaxGroup] = {};
    const int ksize = ds[0].ksize;
    for (int p = 0; p < n; ++p) {
        const EasConvBnActEval* d = &ds[p];
        if (!d->x || !d->packed_w || d->act < 0 || d->act > 1) return EAS_ERR_INVALID_ARG;
        if (d->ksize != ksize || d->stride != 1 || d->x_terms != 3 || (ksize != 1 && ksize != 3)) return EAS_ERR_UNSUPPORTED;
        if (d->Cout % 8 || d->Cin % 8 || d->csplit % 8 || d->csplit < 8 || d->csplit > d->Cout || (ksize == 3 && d->Wi % 2 != 0)) return EAS_ERR_UNSUPPORTED;
        EasBnActEpiDev& b = bna[p];
        b.on = 1; b.act = d->act; b.csplit = d->csplit; b.Cout = d->Cout;
        const int nr = d->csplit < d->Cout ? 2 : 1;
        for (int i = 0; i < nr; ++i) {
            const EasBnActRange& r = d->range[i];
            const int cr = i ? d->Cout - d->csplit : d->csplit;
            if (!r.gamma || !r.beta || !r.mean || !r.invstd || !r.out || r.out_c0 < 0 || r.out_c0 + cr > r.out_ctot) return EAS_ERR_INVALID_ARG;
            if ((((uintptr_t)r.gamma) | ((uintptr_t)r.beta) | ((uintptr_t)r.mean) | ((uintptr_t)r.invstd)) & 15) return EAS_ERR_INVALID_ARG;
            b.r[i] = r;
        }
        if (nr == 1) b.r[1] = b.r[0];
        pr[p].x = d->x; pr[p].packed_w = d->packed_w; pr[p].y = d->range[0].out;
        pr[p].NI = d->NI; pr[p].Cin = d->Cin; pr[p].Cout = d->Cout; pr[p].Hi = d->Hi; pr[p].Wi = d->Wi;
    }
    EAS_CLEAR_ERR();
    const int rc = ksize == 1 ? eas_conv1x1_group(pr, n, 3, eas_s(stream), nullptr, false, bna) : group3_bna(pr, bna, n, eas_s(stream));
    if (rc != EAS_OK) return rc;
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

}  // extern "C"
