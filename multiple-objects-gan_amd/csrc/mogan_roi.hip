// mogan_roi.hip -- the device side of the object-level Frechet distance of DESIGN.md section 9i (SceneFID, Sylvain et al. 2021):
// crop a ragged list of boxes out of a batch of images, compact it and resize every crop to the trunk's input size, in one launch.
// attngan/scenefid.py holds the score's definition; the reference repository has no code for it.
//
// roi_resize_kernel: one thread per output pixel (r, oy, ox); consecutive lanes take consecutive ox, so the stores of a row are
// coalesced and the two source rows a wave reads are near-contiguous.  Taps and weights depend on (r, oy, ox) only and are formed
// once, then the thread walks the C <= 4 channels.  Per axis (x shown), every operation rounded once to fp32, nothing contracted:
//     p0 = box.x * W      pl = box.w * W      scale = pl / OW
//     src(j) = p0 + (((float)j + 0.5f) * scale - 0.5f)      clamped to [0, W - 1]      (a NaN clamps to 0)
//     i0 = floor(src)     i1 = min(i0 + 1, W - 1)           l = src - (float)i0
// so every tap lies inside the image whatever the box holds, and the full box (0, 0, 1, 1) is bilinear interpolation with
// align_corners = False.  A ROI whose w or h is not positive, whose box holds a value that is not finite, or whose image index lies
// outside [0, B) reads nothing of x and gets zeros.  No LDS, no atomics, no workspace; every element of y is written exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

constexpr int NT = 256;
constexpr long long I31 = 2147483647LL;
constexpr int C_MAX = 4;

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

struct Tap {
    int i0, i1;
    float l;
};

// the source coordinate of output position j on an axis of n source and on output pixels, for a box that starts at b0 and is bl long
// (both relative): the definition above, operation by operation
__device__ __forceinline__ Tap tap_of(int j, float b0, float bl, int n, int on) {
    const float p0 = __fmul_rn(b0, (float)n);
    const float pl = __fmul_rn(bl, (float)n);
    const float scale = __fdiv_rn(pl, (float)on);
    float src = __fadd_rn(p0, __fsub_rn(__fmul_rn(__fadd_rn((float)j, 0.5f), scale), 0.5f));
    src = fminf(fmaxf(src, 0.f), (float)(n - 1));                 // fmaxf(NaN, 0) = 0: always inside [0, n - 1]
    Tap t;
    t.i0 = (int)floorf(src);
    t.i1 = min(t.i0 + 1, n - 1);
    t.l = __fsub_rn(src, (float)t.i0);
    return t;
}

__global__ __launch_bounds__(NT) void roi_resize_kernel(const float* __restrict__ x, int B, int C, int H, int W,
                                                        const float* __restrict__ boxes, const int* __restrict__ image_index,
                                                        unsigned total, float* __restrict__ y, int OH, int OW) {
    const unsigned i = blockIdx.x * NT + threadIdx.x;                   // (r, oy, ox); total <= 2^31 - 1: 32-bit divisions
    if (i >= total) return;
    const unsigned t = i / (unsigned)OW;
    const int ox = (int)(i - t * (unsigned)OW);
    const unsigned r = t / (unsigned)OH;
    const int oy = (int)(t - r * (unsigned)OH);
    const size_t plane = (size_t)OH * OW;
    float* out = y + ((size_t)r * C * OH + oy) * OW + ox;
    const float* box = boxes + (size_t)r * 4;
    const float bx = box[0], by = box[1], bw = box[2], bh = box[3];
    const int b = image_index[r];
    const bool finite = isfinite(bx) && isfinite(by) && isfinite(bw) && isfinite(bh);
    if (!finite || !(bw > 0.f) || !(bh > 0.f) || b < 0 || b >= B) {
        for (int c = 0; c < C; ++c) out[c * plane] = 0.f;
        return;
    }
    const Tap tx = tap_of(ox, bx, bw, W, OW), ty = tap_of(oy, by, bh, H, OH);
    const float hx = 1.f - tx.l, hy = 1.f - ty.l;
    const float* p0 = x + ((size_t)b * C * H + ty.i0) * W;
    const float* p1 = x + ((size_t)b * C * H + ty.i1) * W;
    const size_t src_plane = (size_t)H * W;
    for (int c = 0; c < C; ++c) {
        const float top = hx * p0[tx.i0] + tx.l * p0[tx.i1];
        const float bot = hx * p1[tx.i0] + tx.l * p1[tx.i1];
        out[c * plane] = hy * top + ty.l * bot;
        p0 += src_plane;
        p1 += src_plane;
    }
}

}  // namespace

extern "C" int mogan_roi_resize(const float* x, int B, int C, int H, int W, const float* boxes, const int* image_index, long long R,
                                float* y, int OH, int OW, hipStream_t stream) {
    if (!x || !boxes || !image_index || !y) return MOGAN_ERR_SHAPE;
    if (B < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || C < 1 || C > C_MAX || R < 0) return MOGAN_ERR_SHAPE;
    const long long hw = (long long)H * W, ohw = (long long)OH * OW;
    if (hw > I31 || (long long)B > I31 / ((long long)C * hw)) return MOGAN_ERR_SHAPE;
    if (R == 0) return 0;
    if (ohw > I31 || R > I31 / ((long long)C * ohw)) return MOGAN_ERR_SHAPE;
    const long long total = R * ohw;
    roi_resize_kernel<<<dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream>>>(x, B, C, H, W, boxes, image_index,
                                                                                      (unsigned)total, y, OH, OW);
    return ok_launch();
}
