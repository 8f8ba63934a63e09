// Region prompts of image sessions (PSALM.segment(..., regions=...), psalm_amd/model.py): the dataset mapper's host preparation of a click / box /
// scribble prompt (coco_instance_mapper.py:233-252) next to the data, in front of video.hip's psalm_mask_resize_nearest_pad / psalm_mask_select_points:
//   psalm_mask_rasterize     the prompt geometry (pixels, boxes) as (R, h, w) bytes                       bulid_COCO_Interactivate.py:72
//   psalm_mask_dilate_disc   enhance_with_circles: the union of integer discs around every pixel == 1     coco_instance_mapper.py:17-33
//   psalm_region_best        per region the best query (lowest index among equal scores)                  region_segmentation.py:163
//   psalm_mask_gather_u8     the picked queries' binary masks as bytes
// All integer work: results are exact against the host formulas (tests/test_23_prompt_kernels.py).
#include "psalm_hip.h"      // psalm_prompt_prim; the entries below are checked against their declarations
#include "common.h"

#include <climits>

#define PROMPT_MAX_RADIUS 16
#define PROMPT_MAX_Q 1024

// ---------------------------------------------------------------- rasterize
// grid (primitive, row slice).  A pixel is written by thread 0 of slice 0; a box is clipped to the image and its rows are dealt to the slices, a
// row's columns to the threads.  Every writer of a pixel writes 1: no ordering between primitives is needed.
#define RASTER_SLICES 8
__global__ void __launch_bounds__(256) mask_rasterize_kernel(const psalm_prompt_prim* __restrict__ prims, int R, int h, int w,
                                                             unsigned char* __restrict__ masks) {
    const psalm_prompt_prim p = prims[blockIdx.x];
    if (p.region < 0 || p.region >= R) return;
    unsigned char* plane = masks + (long)p.region * h * w;
    if (p.kind == 0) {
        if (blockIdx.y == 0 && threadIdx.x == 0 && p.a >= 0 && p.a < h && p.b >= 0 && p.b < w) plane[(long)p.a * w + p.b] = 1;
        return;
    }
    if (p.kind != 1) return;
    const int y0 = max(p.a, 0), y1 = min(p.c, h), x0 = max(p.b, 0), x1 = min(p.d, w);
    for (int y = y0 + (int)blockIdx.y; y < y1; y += RASTER_SLICES)
        for (int x = x0 + (int)threadIdx.x; x < x1; x += 256) plane[(long)y * w + x] = 1;
}
extern "C" int psalm_mask_rasterize(const psalm_prompt_prim* prims_dev, int n_prims, int R, int h, int w, unsigned char* masks, void* stream) {
    if (R == 0) return 0;
    PSALM_CHECK_ARG(R >= 1 && h >= 1 && w >= 1 && n_prims >= 0, "psalm_mask_rasterize: R >= 1, non-empty planes, n_prims >= 0");
    PSALM_CHECK_ARG(masks != nullptr && (n_prims == 0 || prims_dev != nullptr), "psalm_mask_rasterize: null pointer");
    PSALM_CHECK_ARG(n_prims == 0 || ((uintptr_t)prims_dev & 3) == 0, "psalm_mask_rasterize: the primitive table must be 4-byte aligned");
    if (hipMemsetAsync(masks, 0, (size_t)R * h * w, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_mask_rasterize: hipMemsetAsync failed");
        return -2;
    }
    if (n_prims == 0) return 0;
    hipLaunchKernelGGL(mask_rasterize_kernel, dim3(n_prims, RASTER_SLICES), dim3(256), 0, (hipStream_t)stream, prims_dev, R, h, w, masks);
    PSALM_LAUNCH_END("psalm_mask_rasterize");
}

// ---------------------------------------------------------------- dilation by an integer disc
// Block = a tile of DIL_TH rows x DIL_TW * 64 columns of one plane.  The tile's rows plus `halo` (= max_radius) rows above and below, one 64-bit
// word to the left and right, are staged in LDS as BITS: a wavefront reads 64 consecutive bytes and its __ballot(byte == 1) is one word of a row
// (bit i = column 64 * word + i; 0 outside the plane).  An output word is the OR over dy of the row y + dy dilated horizontally by
// hw(dy) = isqrt(radius^2 - dy^2): shifts by 1 .. hw in both directions, bits carried in from the neighbouring words.  The words are unpacked to
// bytes on store, 64 consecutive bytes per wavefront.  A negative radius copies the tile's bytes unchanged.
#define DIL_TH 32
#define DIL_TW 4
#define DIL_ROWS (DIL_TH + 2 * PROMPT_MAX_RADIUS)
#define DIL_WORDS (DIL_TW + 2)
__global__ void __launch_bounds__(256) mask_dilate_disc_kernel(const unsigned char* __restrict__ in, const int* __restrict__ radius, int max_radius,
                                                               int h, int w, unsigned char* __restrict__ out) {
    __shared__ unsigned long long bits[DIL_ROWS * DIL_WORDS];
    __shared__ unsigned long long res[DIL_TH * DIL_TW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.z, ty0 = blockIdx.y * DIL_TH, tx0 = blockIdx.x * DIL_TW * 64;
    const unsigned char* src = in + (long)r * h * w;
    unsigned char* dst = out + (long)r * h * w;
    int rad = radius[r];
    if (rad < 0) {                                                       // block-uniform: plane r is not dilated
        for (int i = tid; i < DIL_TH * DIL_TW * 64; i += 256) {
            const int y = ty0 + i / (DIL_TW * 64), x = tx0 + i % (DIL_TW * 64);
            if (y < h && x < w) dst[(long)y * w + x] = src[(long)y * w + x];
        }
        return;
    }
    rad = min(rad, max_radius);
    const int halo = max_radius, rows = DIL_TH + 2 * halo;
    for (int i = wave; i < rows * DIL_WORDS; i += 4) {                   // wave-uniform trip count and word: every lane takes part in the ballot
        const int y = ty0 - halo + i / DIL_WORDS, x = tx0 + (i % DIL_WORDS - 1) * 64 + lane;
        const bool seed = y >= 0 && y < h && x >= 0 && x < w && src[(long)y * w + x] == 1;
        const unsigned long long word = __ballot(seed ? 1 : 0);
        if (lane == 0) bits[i] = word;
    }
    __syncthreads();
    if (tid < DIL_TH * DIL_TW) {
        const int ry = tid / DIL_TW, wx = tid % DIL_TW;
        unsigned long long acc = 0;
        for (int dy = -rad; dy <= rad; ++dy) {
            const unsigned long long* row = bits + (ry + halo + dy) * DIL_WORDS + wx;       // [left | centre | right]
            const unsigned long long lw = row[0], cw = row[1], rw = row[2];
            if ((lw | cw | rw) == 0ull) continue;
            int hw = 0;
            while ((hw + 1) * (hw + 1) + dy * dy <= rad * rad) ++hw;
            acc |= cw;
            for (int s = 1; s <= hw; ++s) acc |= (cw << s) | (lw >> (64 - s)) | (cw >> s) | (rw << (64 - s));
        }
        res[tid] = acc;
    }
    __syncthreads();
    for (int i = wave; i < DIL_TH * DIL_TW; i += 4) {
        const int y = ty0 + i / DIL_TW, x = tx0 + (i % DIL_TW) * 64 + lane;
        if (y < h && x < w) dst[(long)y * w + x] = (unsigned char)((res[i] >> lane) & 1ull);
    }
}
extern "C" int psalm_mask_dilate_disc(const unsigned char* in, const int* radius_dev, int max_radius, int R, int h, int w, unsigned char* out,
                                      void* stream) {
    if (R == 0) return 0;
    PSALM_CHECK_ARG(max_radius >= 0 && max_radius <= PROMPT_MAX_RADIUS, "psalm_mask_dilate_disc: 0 <= max_radius <= 16");
    PSALM_CHECK_ARG(R >= 1 && R <= 65535 && h >= 1 && w >= 1 && (long)h * w <= INT_MAX, "psalm_mask_dilate_disc: 1 <= R <= 65535, 1 <= h * w < 2^31");
    PSALM_CHECK_ARG(in != nullptr && out != nullptr && radius_dev != nullptr, "psalm_mask_dilate_disc: null pointer");
    PSALM_CHECK_ARG(in != out, "psalm_mask_dilate_disc: in == out (a tile reads its neighbours' input)");
    const int gx = cdiv(w, DIL_TW * 64), gy = cdiv(h, DIL_TH);
    PSALM_CHECK_ARG(gy <= 65535, "psalm_mask_dilate_disc: at most 65535 * 32 rows");
    hipLaunchKernelGGL(mask_dilate_disc_kernel, dim3(gx, gy, R), dim3(256), 0, (hipStream_t)stream, in, radius_dev, max_radius, h, w, out);
    PSALM_LAUNCH_END("psalm_mask_dilate_disc");
}

// ---------------------------------------------------------------- the best query of every region
// scores (Q, R): region r's candidates are column r.  One wavefront per region; a lane walks its queries in ascending order and keeps a strictly
// greater score, the butterfly prefers the lower query among equal scores: the first occurrence of the maximum, as video_pick_kernel ranks.
__global__ void __launch_bounds__(64) region_best_kernel(const float* __restrict__ scores, int Q, int R, int* __restrict__ best_query,
                                                         float* __restrict__ best_score) {
    const int r = blockIdx.x, lane = threadIdx.x;
    int bi = -1;
    float bv = 0.f;
    for (int q = lane; q < Q; q += 64) {
        const float v = scores[(long)q * R + r];
        if (bi < 0 || v > bv) { bi = q; bv = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oi = __shfl_xor(bi, o);
        const float ov = __shfl_xor(bv, o);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bi = oi; bv = ov; }
    }
    if (lane == 0) {
        best_query[r] = bi;
        best_score[r] = bv;
    }
}
extern "C" int psalm_region_best(const float* scores, int Q, int R, int* best_query, float* best_score, void* stream) {
    PSALM_CHECK_ARG(Q >= 1 && Q <= PROMPT_MAX_Q && R >= 1, "psalm_region_best: 1 <= Q <= 1024, R >= 1");
    PSALM_CHECK_ARG(scores != nullptr && best_query != nullptr && best_score != nullptr, "psalm_region_best: null pointer");
    hipLaunchKernelGGL(region_best_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, scores, Q, R, best_query, best_score);
    PSALM_LAUNCH_END("psalm_region_best");
}

// ---------------------------------------------------------------- the picked queries' masks as bytes
// out[r][p] = masks[query[r]][p] > 0 (psalm_binarize_gather's test, one byte per pixel); a query outside [0, Q) gives an empty mask.
__global__ void __launch_bounds__(256) mask_gather_u8_kernel(const float* __restrict__ masks, const int* __restrict__ query, int Q, long HW,
                                                             unsigned char* __restrict__ out) {
    const int r = blockIdx.y, q = query[r];
    const bool ok = q >= 0 && q < Q;
    const float* src = masks + (long)(ok ? q : 0) * HW;
    unsigned char* dst = out + (long)r * HW;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256) dst[p] = (ok && src[p] > 0.f) ? 1 : 0;
}
extern "C" int psalm_mask_gather_u8(const float* masks, const int* query, int Q, int R, long HW, unsigned char* out, void* stream) {
    if (R == 0 || HW == 0) return 0;
    PSALM_CHECK_ARG(Q >= 1 && R >= 1 && R <= 65535 && HW >= 1, "psalm_mask_gather_u8: Q >= 1, 1 <= R <= 65535, HW >= 1");
    PSALM_CHECK_ARG(masks != nullptr && query != nullptr && out != nullptr, "psalm_mask_gather_u8: null pointer");
    const long gx = (HW + 1023) / 1024;
    hipLaunchKernelGGL(mask_gather_u8_kernel, dim3((unsigned)(gx > 4096 ? 4096 : gx), R), dim3(256), 0, (hipStream_t)stream, masks, query, Q, HW, out);
    PSALM_LAUNCH_END("psalm_mask_gather_u8");
}
