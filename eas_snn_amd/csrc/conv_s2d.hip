// Input gradient of a stride-2 3x3 convolution with the four parity classes of the gx pixel in ONE tile (round 5).
//
// Until round 5 every parity class (ph, pw) of the gx pixel ran as a stride-1 tap-list convolution of its own ("class kernels", since
// removed): each staged grad_y by itself -- the three-term split of a staged element (about ten vector instructions) then fed ONE tap in
// class (0, 0) against nine in a forward tile -- and each wrote every second pixel of every second row of gx, so that a 128-byte line of gx
// was put together by four blocks on four XCDs.  Measured then (config 2, scripts/dev_conv_calls_table.py): 2.0x the time of a stride-1
// input gradient of the same MFMA work.
//
// A block stages its grad_y patch once (rows a .. a + 1, columns b .. b + 1 of its positions, 16 channels per chunk, three terms) and
// walks the nine taps of a chunk like a forward 3x3 tile; tap t accumulates into the accumulators of its class (conv_tile_body NC = 4), a
// wave holds 4 classes x WN position tiles (WN = 2: 128 accumulator registers), and the epilogue writes gx[2a + ph][2b .. 2b + 1] as one
// 8-byte store per lane: whole lines from one block.  Per accumulator the products arrive in the order of the class kernels (k-step major,
// the class's taps, smallest term products first), so the result is bit-identical to theirs.  Weights: the mode-2 pack, unchanged.
//
// Tiles are ragged over the rows of an image (conv_mfma_body.h bpi) where whole images do not fill the 32 * WN * WVN positions of a block:
// 3 rows of 40 / 6 rows of 20 positions in a 128-position tile.
#include "conv_mfma_body.h"

namespace {

// VEC = 1: a staging item is ONE position x 8 channels (eight 4-byte loads, coalesced over the lanes' consecutive positions; one 16-byte LDS
// store per term), up to four items per thread: the conversion work of a chunk is spread over every lane of the block and over the last
// steps of the chunk instead of sitting in the first one or two waves behind the last step.
template <int VEC>
constexpr int s2c_nit() { return VEC == 1 ? 4 : 1; }

template <int WN, int WVM, int WVN, int VEC>
__global__ __launch_bounds__(64 * WVM * WVN, 2) void conv_dgrad_s2c_kernel(const float* __restrict__ gy, const bf16x8* __restrict__ wp,
                                                                             float* __restrict__ gx, const ConvGeomCore g) {
    extern __shared__ __align__(16) unsigned char smem[];
    conv_tile_body<9, 1, 3, 1, WN, WVM, WVN, 16, VEC, s2c_nit<VEC>(), false, 0, ConvGeomCore, 4>(gy, wp, nullptr, gx, nullptr, g, 0, smem,
                                                                                                (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x);
}

template <int WN, int WVM, int WVN, int VEC>
int launch_s2c(const float* gy, const bf16x8* wp, float* gx, ConvGeomCore g, size_t lds, hipStream_t st) {
    auto kern = conv_dgrad_s2c_kernel<WN, WVM, WVN, VEC>;
    static bool attr_set = false;
    if (const int rc = conv_launch_prep((const void*)kern, attr_set, g, VEC, 16)) return rc;
    EAS_LAUNCH(kern, conv_tile_grid(g, WVM), dim3(64 * WVM * WVN), lds, st, gy, wp, gx, g);
    return EAS_OK;
}

typedef int (*s2c_fn)(const float*, const bf16x8*, float*, ConvGeomCore, size_t, hipStream_t);
struct S2cCand { int wvm, wvn, wn, threads; s2c_fn f4, f2, f1; };
#define EAS_S2C(WVM_, WVN_, WN_) {WVM_, WVN_, WN_, 64 * WVM_ * WVN_, launch_s2c<WN_, WVM_, WVN_, 4>, launch_s2c<WN_, WVM_, WVN_, 2>, launch_s2c<WN_, WVM_, WVN_, 1>}
const S2cCand kS2c[7] = {EAS_S2C(2, 4, 2), EAS_S2C(4, 2, 2), EAS_S2C(2, 2, 2), EAS_S2C(4, 1, 2), EAS_S2C(1, 4, 2), EAS_S2C(4, 1, 1), EAS_S2C(2, 2, 1)};
#undef EAS_S2C

// grad_y [NI, Cout, Ho, Wo] -> grad_x [NI, Cin, Hi, Wi]; packed_w: mode 2.  EAS_ERR_UNSUPPORTED: no tile -- odd Wo, Cout no multiple of 8,
// rows wider than the widest candidate (Wo > 256), total rows beyond the fdiv range -- and nothing is launched.  query: plan only.
int dgrad_s2_plan(const float* gy, const void* packed_w, float* gx, int NI, int Cin, int Cout, int Hi, int Wi, hipStream_t st, bool query) {
    const int Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1;
    if (Cout % 8 != 0 || Wo % 2 != 0) return EAS_ERR_UNSUPPORTED;
    static const int force_vec = eas_dev_env("EAS_S2C_VEC") ? atoi(eas_dev_env("EAS_S2C_VEC")) : 0;      // development: 2 = 8-byte staging loads everywhere
    // staging items of 2 positions x 8 channels where a chunk's items fit the block's threads (measured 3-6 % faster than 4 positions: more
    // lanes share the conversion work), else 4 positions, else single positions (four items per thread)
    const int vec_pref[3] = {2, Wo % 4 == 0 ? 4 : 0, 1};
    ConvGeomCore g{};
    g.NI = NI; g.Cin = Cout; g.Cout = Cin; g.Hi = Ho; g.Wi = Wo; g.Ho = Ho; g.Wo = Wo;
    g.RS = Wo + 1;                      // one zero column right of the image: position b + 1 of the last column
    g.pad_t = g.pad_l = 0;
    g.ext_h = 2;                        // rows a and a + 1
    for (int t = 0; t < 9; ++t) {       // class-major taps: class 2 * ph + pw, its taps (ih, iw) with ih <= ph, iw <= pw
        const int cls = kS2Cls[t], pw = cls & 1, lt = kS2Lt[t];
        const int ih = lt / (pw + 1), iw = lt - ih * (pw + 1);
        g.tap_off[t] = ih * g.RS + iw;
    }
    g.oH = Hi; g.oW = Wi; g.os = 2; g.oph = g.opw = 0;
    g.MT = (Cin + 31) / 32; g.KSTEPS = (Cout + 15) / 16;
    g.total_rows = NI * Ho;
    g.Wst = Wo; g.gx0 = 0; g.qshift = 0; g.parts = 1;
    g.dbg = conv_dev_dbg();
    const int nbuf = g.KSTEPS <= 1 ? 1 : 2;
    int best = -1, best_vec = 0;
    double best_cost = 0.0;
    size_t best_lds = 0;
    ConvGeomCore best_g = g;
    static const int force = eas_dev_env("EAS_S2C_TILE") ? atoi(eas_dev_env("EAS_S2C_TILE")) : -1;      // development: force a candidate
    for (int i = 0; i < 7; ++i) {
        const S2cCand& c = kS2c[i];
        if (force >= 0 && i != force) continue;
        if ((c.wvm - 1) * 32 >= Cin) continue;
        ConvGeomCore t = g;
        const int bn = 32 * c.wn * c.wvn;
        // ragged tiles, ONE attempt at the candidate's full pixel count (no shrinking: a narrower candidate follows), and the staging width
        // chosen afterwards: the first preference whose items fit -- one item per thread, four for single positions (s2c_nit)
        if (bn < Wo || !conv_tile_rows(t, bn, 1, true)) continue;
        size_t lds = 0;
        int vec = 0;
        for (int k = 0; k < 3 && !vec; ++k) {
            const int v = vec_pref[k];
            if (!v || (force_vec != 0 && force_vec != v) || Wo % v != 0) continue;
            lds = conv_tile_fit(t, nbuf, 16, 3, v, (v == 1 ? 4 : 1) * c.threads);
            if (lds) vec = v;
        }
        if (!vec) continue;
        const dim3 grid = conv_tile_grid(t, c.wvm);
        const long blocks = (long)grid.x * grid.y;
        const int bpc = conv_blocks_per_cu(c.threads, lds);
        // the forward tiles' round cost (conv_mfma_body.h) with the MFMA work of a wave relative to WN = 2 and no latency floor (the model
        // this kernel was tuned with; a floor has not been measured here)
        const double round_cost = conv_round_factor(c.threads, bpc, (double)blocks) * conv_block_time(c.wn, 2.0, 192.0, 0.0);
        const double cost = (double)((blocks + 256 * bpc - 1) / (256 * bpc)) * round_cost;
        if (best < 0 || cost < best_cost - 1e-9) {
            best = i; best_cost = cost; best_g = t; best_vec = vec; best_lds = lds;
        }
    }
    if (best < 0) return EAS_ERR_UNSUPPORTED;
    conv_plan_note("s2c", best, kS2c[best].wvm, kS2c[best].wvn, kS2c[best].wn, best_vec, best_g, conv_tile_grid(best_g, kS2c[best].wvm), best_lds);
    if (query) return EAS_OK;
    const s2c_fn fn = best_vec == 4 ? kS2c[best].f4 : (best_vec == 2 ? kS2c[best].f2 : kS2c[best].f1);
    return fn(gy, (const bf16x8*)packed_w, gx, best_g, best_lds, st);
}

}  // namespace

extern "C" {

// grad_x[NI,Cin,Hi,Wi] of a stride-2 3x3 convolution (padding 1) from grad_y[NI,Cout,Ho,Wo] (general fp32, three bf16 terms) and the
// weights packed with mode 2: one launch.  Refused geometries (eas_conv_dgrad_s2_supported = 0) launch nothing and leave grad_x alone.
int eas_conv_dgrad_s2(const float* grad_y, const void* packed_w, float* grad_x, int NI, int Cin, int Cout, int Hi, int Wi, eas_stream_t stream) {
    if (!grad_y || !packed_w || !grad_x || NI <= 0 || Cin <= 0 || Cout <= 0 || Hi <= 0 || Wi <= 0) return EAS_ERR_INVALID_ARG;
    EAS_CLEAR_ERR();
    const int rc = dgrad_s2_plan(grad_y, packed_w, grad_x, NI, Cin, Cout, Hi, Wi, eas_s(stream), false);
    if (rc != EAS_OK) return rc;
    EAS_CHECK_LAUNCH();
    return EAS_OK;
}

// 1 when eas_conv_dgrad_s2 has a tile for this geometry (the same plan, nothing launched), else 0
int eas_conv_dgrad_s2_supported(int NI, int Cin, int Cout, int Hi, int Wi) {
    if (NI <= 0 || Cin <= 0 || Cout <= 0 || Hi <= 0 || Wi <= 0) return 0;
    return dgrad_s2_plan(nullptr, nullptr, nullptr, NI, Cin, Cout, Hi, Wi, nullptr, true) == EAS_OK ? 1 : 0;
}

// the tile eas_conv_dgrad_s2 launches for this geometry, as the plan left it at its exit: the launch's status, *out filled when EAS_OK
int eas_conv_dgrad_s2_plan(int NI, int Cin, int Cout, int Hi, int Wi, EasConvPlan* out) {
    if (!out || NI <= 0 || Cin <= 0 || Cout <= 0 || Hi <= 0 || Wi <= 0) return EAS_ERR_INVALID_ARG;
    const int rc = dgrad_s2_plan(nullptr, nullptr, nullptr, NI, Cin, Cout, Hi, Wi, nullptr, true);
    if (rc == EAS_OK) *out = tl_conv_plan[0];
    return rc;
}

}  // extern "C"
