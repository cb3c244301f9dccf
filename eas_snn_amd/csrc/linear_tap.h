// cv2.resize(INTER_LINEAR) along one axis: the one statement of the rule for every kernel that resizes count frames
// (events.hip counts_letterbox_kernel, stacked_hist.hip stacked_hist_frames_kernel).  Restated from OpenCV's resize.cpp (not in the
// reference tree, opencv-python pinned by pip-requirements.txt; no cv2 in this image: parity unpinned):
// fx = float((j + 0.5) * (n_src / n_dst) - 0.5), sx = floor(fx), fx -= sx, clamped at both borders with fx = 0; float32 weights.
// The callers multiply in float64, horizontal pass first: out = (S[sy][sx]*a0 + S[sy][sx+1]*a1)*b0 + (...)*b1.
#pragma once
#include <hip/hip_runtime.h>

struct AxisTap { int s0, s1; float w0, w1; };

// tap of destination index j (0 <= j < n_dst, n_src >= 1): 0 <= s0 <= s1 <= n_src - 1 for every such j
__device__ __forceinline__ AxisTap linear_tap(int j, int n_src, int n_dst) {
    const double scale = (double)n_src / (double)n_dst;
    float f = (float)(((double)j + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    AxisTap t;
    t.s0 = s;
    t.s1 = s + 1 < n_src ? s + 1 : n_src - 1;
    t.w0 = 1.f - f;
    t.w1 = f;
    return t;
}
