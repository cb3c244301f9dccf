// Resize / paste / flip of count frames: the one statement of the rule for every kernel that does it (events.hip counts_letterbox_kernel,
// stacked_hist.hip stacked_hist_frames_kernel).  A front end with another interpolation adds a tap function and nothing else.
//
// cv2.resize for float64 images, restated from OpenCV's resize.cpp (not in the reference tree, opencv-python pinned by pip-requirements.txt;
// no cv2 in this image: parity unpinned).  Per axis f = float((j + 0.5) * (n_src / n_dst) - 0.5), s = floor(f), f -= s; float32 weights;
// float64 arithmetic, horizontal pass first, the products of a pass added left to right, then the cast to fp32.
//   INTER_LINEAR (gen1.py:433-521, rvt_gen4.py:510-598): taps s, s + 1, clamped at both borders with f = 0
//   INTER_CUBIC  (NCaltech.batch_resize, ncaltech.py:98-105, 293-295, 313, 342): taps s - 1 .. s + 2 without a clamp of f, each index
//                clamped to the image, weights with A = -0.75 (interpolateCubic)
// No FMA contraction anywhere (this library is built with -ffp-contract=off; the pragmas say so for these functions whatever the flags), so
// the result equals a numpy restatement bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// source indices and weights of one destination index along one axis
template <int N>
struct Taps { int s[N]; float c[N]; };

// taps of destination index j (0 <= j < n_dst, n_src >= 1): 0 <= s[k] <= n_src - 1 for every such j, both rules
__device__ __forceinline__ Taps<2> linear_tap(int j, int n_src, int n_dst) {
    const double scale = (double)n_src / (double)n_dst;
    float f = (float)(((double)j + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    Taps<2> t;
    t.s[0] = s;
    t.s[1] = s + 1 < n_src ? s + 1 : n_src - 1;
    t.c[0] = 1.f - f;
    t.c[1] = f;
    return t;
}

__device__ __forceinline__ Taps<4> cubic_tap(int j, int n_src, int n_dst) {
#pragma clang fp contract(off)
    const double scale = (double)n_src / (double)n_dst;
    float f = (float)(((double)j + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    const float A = -0.75f;
    Taps<4> t;
    t.c[0] = ((A * (f + 1.f) - 5.f * A) * (f + 1.f) + 8.f * A) * (f + 1.f) - 4.f * A;
    t.c[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
    t.c[2] = ((A + 2.f) * (1.f - f) - (A + 3.f)) * (1.f - f) * (1.f - f) + 1.f;
    t.c[3] = 1.f - t.c[0] - t.c[1] - t.c[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = s - 1 + k;
        t.s[k] = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);
    }
    return t;
}

// the tap rule as a type, for kernels templated on it
struct LinearRule {
    static constexpr int N = 2;
    static __device__ __forceinline__ Taps<2> tap(int j, int n_src, int n_dst) { return linear_tap(j, n_src, n_dst); }
};
struct CubicRule {
    static constexpr int N = 4;
    static __device__ __forceinline__ Taps<4> tap(int j, int n_src, int n_dst) { return cubic_tap(j, n_src, n_dst); }
};

// One destination value: row(y) points to source row y (integer counts), so a row's address is formed once for its N taps (one thread
// per pixel with 16 taps: 4 % of the cubic letterbox, profiles/resize_one_rule_ab.txt).  N = 2: (S[y0][x0]*a0 + S[y0][x1]*a1)*b0 + (...)*b1.
template <int N, typename Row>
__device__ __forceinline__ float resample(Row row, const Taps<N>& tx, const Taps<N>& ty) {
#pragma clang fp contract(off)
    double rows[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const auto r = row(ty.s[k]);
        double a = (double)r[tx.s[0]] * (double)tx.c[0];
#pragma unroll
        for (int m = 1; m < N; ++m) a = a + (double)r[tx.s[m]] * (double)tx.c[m];
        rows[k] = a;
    }
    double v = rows[0] * (double)ty.c[0];
#pragma unroll
    for (int k = 1; k < N; ++k) v = v + rows[k] * (double)ty.c[k];
    return (float)v;
}

// Where the resized frame lies on the canvas: a params row (nw, nh, dx, dy, flip) -- the frame resized to nw x nh, its top left corner at
// (dx, dy), then the canvas mirrored left-right --, or none: the W x H sensor unscaled at the top left.  The row is device data nobody has
// validated: the rectangle is whatever part of [dx, dx + nw) x [dy, dy + nh) lies on the canvas, and nw <= 0 or nh <= 0 is an empty one.
struct Paste {
    int nw, nh, dx, dy, flip;

    __device__ __forceinline__ explicit Paste(const int32_t* __restrict__ row) : nw(row[0]), nh(row[1]), dx(row[2]), dy(row[3]), flip(row[4]) {}
    __device__ __forceinline__ Paste(int W, int H) : nw(W), nh(H), dx(0), dy(0), flip(0) {}          // no row
    // Column / row of the resized frame under canvas column xx / row yy (both >= 0); outside the frame unless has_col / has_row.  The
    // difference wraps at 32 bits, which those tests survive for any dx, dy: the true value lies in (-2^31, 2^32), and from 2^31 on -- right
    // of every frame -- it wraps to a negative one.
    __device__ __forceinline__ int src_col(int xx, int Wc) const { return (int)((uint32_t)(flip ? Wc - 1 - xx : xx) - (uint32_t)dx); }
    __device__ __forceinline__ int src_row(int yy) const { return (int)((uint32_t)yy - (uint32_t)dy); }
    __device__ __forceinline__ bool has_col(int xs) const { return xs >= 0 && xs < nw; }
    __device__ __forceinline__ bool has_row(int ys) const { return ys >= 0 && ys < nh; }
    __device__ __forceinline__ bool inside(int xs, int ys) const { return has_col(xs) && has_row(ys); }
    // cv2.resize with dsize == size is a copy
    __device__ __forceinline__ bool identity(int W, int H) const { return nw == W && nh == H; }
    // does any pixel of canvas rows [y0, y0 + rows), all Wc columns, lie inside the frame
    __device__ __forceinline__ bool touches(int y0, int rows, int Wc) const {
        return nw > 0 && nh > 0 && (int64_t)y0 + rows - 1 >= dy && (int64_t)y0 - dy < nh && (int64_t)dx < Wc && (int64_t)dx + nw > 0;
    }
};
