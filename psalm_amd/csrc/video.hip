// Video object tracking (psalm_amd/video.py): the per-frame bookkeeping of the reference's DAVIS driver (psalm/eval/eval_davis.py:388-480, --with_memory)
// next to the data instead of on the host after pulling all Q full-resolution masks across the bus:
//   psalm_video_pick                one query per object from its ten best scores, skipping queries already taken              eval_davis.py:443-457
//   psalm_video_fuse                the picked masks as bytes, the DAVIS label map, pairwise intersection / union counts and the
//                                   memory_correct_flag (no pair with IoU > 0.4)                                               eval_davis.py:337-342, 458-473
//   psalm_mask_resize_nearest_pad   transforms.apply_segmentation of the memory masks (Pillow NEAREST + zero pad) through host-built
//                                   source-index tables, with per-row set-pixel counts                                         eval_davis.py:406-408
//   psalm_mask_select_points        the sampled rows of mask.nonzero() / [H, W] without materialising nonzero()                context_cluster.py:345-356
// All integer work except the final correctly rounded fp32 division: results are exact against the host formulas (tests/test_13_video_kernels.py).
#include "common.h"

#include <climits>

#define VIDEO_MAX_R 32              // objects per frame: one bit each in a 32-bit per-pixel set
#define VIDEO_MAX_Q 1024
#define VIDEO_TOPK 10               // torch.topk(cur_scores, 10), eval_davis.py:446

// ---------------------------------------------------------------- pick: sequential over objects -> one wavefront
// scores (Q, R): object r's candidates are column r.  Its ten best in descending order (equal scores: lowest query first; scores are NaN-free
// products of sigmoids); the first one no earlier object took is its pick.  An object whose ten best are all taken keeps the PREVIOUS object's pick
// and takes nothing (the reference's loop leaves pick_idx / pick_score as they were, eval_davis.py:448-456); object 0 always finds one.
__global__ void __launch_bounds__(64) video_pick_kernel(const float* __restrict__ scores, int Q, int R, int* __restrict__ pick_query,
                                                        float* __restrict__ pick_score) {
    __shared__ unsigned char taken[VIDEO_MAX_Q], listed[VIDEO_MAX_Q];
    const int lane = threadIdx.x;
    for (int q = lane; q < Q; q += 64) taken[q] = 0;
    __syncthreads();
    int cur_q = 0;
    float cur_s = 0.f;
    for (int r = 0; r < R; ++r) {
        for (int q = lane; q < Q; q += 64) listed[q] = 0;
        __syncthreads();
        bool found = false;
        for (int k = 0; k < VIDEO_TOPK && !found; ++k) {            // (`found` is wave-uniform: every lane holds the same reduced candidate)
            int bi = -1;
            float bv = 0.f;
            for (int q = lane; q < Q; q += 64) {
                if (listed[q]) continue;
                const float v = scores[(long)q * R + r];
                if (bi < 0 || v > bv) { bi = q; bv = v; }              // ascending q: a tie keeps the lower index
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int oi = __shfl_xor(bi, o);
                const float ov = __shfl_xor(bv, o);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bi = oi; bv = ov; }
            }
            if (bi < 0) break;                                         // fewer than ten candidates (the entry refuses Q < 10)
            if (!taken[bi]) { found = true; cur_q = bi; cur_s = bv; }
            __syncthreads();
            if (lane == 0) {
                listed[bi] = 1;
                if (found) taken[bi] = 1;
            }
            __syncthreads();
        }
        if (lane == 0) {
            pick_query[r] = cur_q;
            pick_score[r] = cur_s;
        }
    }
}
extern "C" int psalm_video_pick(const float* scores, int Q, int R, int* pick_query, float* pick_score, void* stream) {
    PSALM_CHECK_ARG(Q >= VIDEO_TOPK && Q <= VIDEO_MAX_Q, "psalm_video_pick: 10 <= Q <= 1024 (the pick reads each object's ten best scores)");
    PSALM_CHECK_ARG(R >= 1 && R <= VIDEO_MAX_R, "psalm_video_pick: 1 <= R <= 32 objects");
    hipLaunchKernelGGL(video_pick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scores, Q, R, pick_query, pick_score);
    PSALM_LAUNCH_END("psalm_video_pick");
}

// ---------------------------------------------------------------- fuse
// One pass over the pixels.  A wavefront takes 64 consecutive pixels; every lane forms the bit set of the R picked masks at its pixel, writes the R
// mask bytes and the label (objects are painted in index order: the highest set bit's fill number stays).  Pair counts: lane r (< R) keeps the
// wavefront's ballot of bit r; ballot i is broadcast and lane j adds popcount(ballot_i & ballot_j) to its register acc[i] = co[i][j], the number of
// pixels set in both mask i and mask j (co[i][i]: pixels of mask i).  Wave registers -> block partial in LDS -> one integer atomic per non-zero
// cell and block into `co` (32 x 32, zeroed by the entry): integer sums, independent of arrival order.
// A mask element counts as set when it is non-zero (the input is psalm_binarize_gather's 0 / 1).
__global__ void __launch_bounds__(256) video_fuse_kernel(const float* __restrict__ pred, const int* __restrict__ pick, const int* __restrict__ fill,
                                                         int Q, int R, long HW, unsigned char* __restrict__ picked, unsigned char* __restrict__ fused,
                                                         int* __restrict__ co) {
    __shared__ unsigned part[VIDEO_MAX_R * VIDEO_MAX_R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < VIDEO_MAX_R * VIDEO_MAX_R; i += 256) part[i] = 0;
    __syncthreads();
    unsigned acc[VIDEO_MAX_R];
#pragma unroll
    for (int i = 0; i < VIDEO_MAX_R; ++i) acc[i] = 0;
    for (long base = ((long)blockIdx.x * 4 + wave) * 64; base < HW; base += (long)gridDim.x * 256) {      // wave-uniform trip count
        const long p = base + lane;
        const bool in = p < HW;
        unsigned bits = 0;
        unsigned label = 0;
        unsigned long long mine = 0;
        for (int r = 0; r < R; ++r) {
            const int q = pick[r];
            const bool set = in && (unsigned)q < (unsigned)Q && pred[(long)q * HW + p] != 0.f;
            if (in) picked[(long)r * HW + p] = set ? 1 : 0;
            if (set) { bits |= 1u << r; label = (unsigned)fill[r]; }
            const unsigned long long b = __ballot(set ? 1 : 0);
            if (lane == r) mine = b;
        }
        if (in) fused[p] = (unsigned char)label;
        if (__ballot(bits != 0) == 0ull) continue;                     // wave-uniform: no object in these 64 pixels
#pragma unroll
        for (int i = 0; i < VIDEO_MAX_R; ++i) {
            if (i < R) {                                               // wave-uniform
                const unsigned long long bi = __shfl(mine, i);
                acc[i] += (unsigned)__builtin_popcountll(bi & mine);
            }
        }
    }
    if (lane < R) {
#pragma unroll
        for (int i = 0; i < VIDEO_MAX_R; ++i)
            if (i < R && acc[i]) atomicAdd(&part[i * VIDEO_MAX_R + lane], acc[i]);
    }
    __syncthreads();
    for (int i = tid; i < VIDEO_MAX_R * VIDEO_MAX_R; i += 256)
        if (part[i]) atomicAdd(&co[i], (int)part[i]);
}
// co -> inter (R, R), union (R, R), nonzero (R), flag.  inter[i][j] = co[i][j]; union = |i| + |j| - inter.  flag = 1 unless some i != j has
// inter / union > 0.4 as numpy evaluates it in float64: for integers that is 5 * inter > 2 * union exactly (at inter / union == 2 / 5 the float64
// quotient is the double nearest 0.4, i.e. the literal itself: not greater; union == 0 gives NaN, not greater either, and 0 > 0 is false here).
__global__ void __launch_bounds__(256) video_fuse_finish_kernel(const int* __restrict__ co, int R, int* __restrict__ inter, int* __restrict__ uni,
                                                                int* __restrict__ nonzero, int* __restrict__ flag) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < R * R; t += 256) {
        const int i = t / R, j = t % R;
        const long long in = co[i * VIDEO_MAX_R + j];
        const long long un = (long long)co[i * VIDEO_MAX_R + i] + co[j * VIDEO_MAX_R + j] - in;
        inter[t] = (int)in;
        uni[t] = (int)un;
        if (i == j) nonzero[i] = (int)in;
        else if (5ll * in > 2ll * un) atomicAdd(&bad, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) flag[0] = bad ? 0 : 1;
}
extern "C" long psalm_video_fuse_workspace(int R) {
    return (R >= 1 && R <= VIDEO_MAX_R) ? (long)VIDEO_MAX_R * VIDEO_MAX_R * 4 : -1;
}
extern "C" int psalm_video_fuse(const float* pred_masks, const int* pick_query, const int* fill, int Q, int R, long HW, unsigned char* picked,
                                unsigned char* fused, int* inter, int* uni, int* nonzero, int* flag, void* workspace, long workspace_bytes,
                                void* stream) {
    PSALM_CHECK_ARG(R >= 1 && R <= VIDEO_MAX_R, "psalm_video_fuse: 1 <= R <= 32 objects");
    PSALM_CHECK_ARG(Q >= 1 && HW >= 1 && HW <= INT_MAX, "psalm_video_fuse: Q >= 1, 1 <= HW < 2^31 (the pixel counts are int32)");
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_video_fuse_workspace(R) && ((uintptr_t)workspace & 3) == 0,
                    "psalm_video_fuse: workspace of psalm_video_fuse_workspace(R) bytes, 4-byte aligned");
    int* co = (int*)workspace;
    if (hipMemsetAsync(co, 0, (size_t)VIDEO_MAX_R * VIDEO_MAX_R * 4, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_video_fuse: hipMemsetAsync failed");
        return -2;
    }
    const long gx = (HW + 255) / 256;
    hipLaunchKernelGGL(video_fuse_kernel, dim3((unsigned)(gx > 1024 ? 1024 : gx)), dim3(256), 0, (hipStream_t)stream, pred_masks, pick_query, fill, Q, R,
                       HW, picked, fused, co);
    hipLaunchKernelGGL(video_fuse_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)co, R, inter, uni, nonzero, flag);
    PSALM_LAUNCH_END("psalm_video_fuse");
}

// ---------------------------------------------------------------- nearest resize + zero pad through source-index tables
// out[r][y][x] = in[r][row_tab[y]][col_tab[x]], 0 where either table entry is negative (a pad position).  The tables hold what Pillow's NEAREST
// resampler reads (psalm_amd/preprocess.py nearest_pad_tables): no index arithmetic here.  Block = one output row of one mask; row_cnt[r][y] = set
// (non-zero) pixels of that row, also added to total[r] when given (zeroed by the caller; integer atomic).
__global__ void __launch_bounds__(256) mask_resize_nearest_pad_kernel(const unsigned char* __restrict__ in, int h, int w, const int* __restrict__ row_tab,
                                                                      const int* __restrict__ col_tab, int Sh, int Sw, unsigned char* __restrict__ out,
                                                                      int* __restrict__ row_cnt, int* __restrict__ total) {
    __shared__ int wsum[4];
    const int y = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int sy = row_tab[y];
    const unsigned char* src = in + ((long)r * h + (sy >= 0 && sy < h ? sy : 0)) * w;
    unsigned char* dst = out + ((long)r * Sh + y) * Sw;
    int c = 0;
    for (int x0 = 0; x0 < Sw; x0 += 256) {                              // block-uniform trip count (the ballot below needs whole wavefronts)
        const int x = x0 + tid;
        unsigned char v = 0;
        if (x < Sw) {
            const int sx = col_tab[x];
            if (sy >= 0 && sy < h && sx >= 0 && sx < w) v = src[sx];
            dst[x] = v;
        }
        c += __builtin_popcountll(__ballot(v != 0 ? 1 : 0));
    }
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        const int n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        row_cnt[(long)r * Sh + y] = n;
        if (total != nullptr && n) atomicAdd(&total[r], n);
    }
}
extern "C" int psalm_mask_resize_nearest_pad(const unsigned char* in, int R, int h, int w, const int* row_tab, const int* col_tab, int Sh, int Sw,
                                             unsigned char* out, int* row_cnt, int* total_zeroed, void* stream) {
    if (R == 0) return 0;
    PSALM_CHECK_ARG(R >= 1 && R <= 65535 && h >= 1 && w >= 1 && Sh >= 1 && Sw >= 1, "psalm_mask_resize_nearest_pad: 1 <= R <= 65535, non-empty geometry");
    PSALM_CHECK_ARG((long)Sh * Sw <= INT_MAX, "psalm_mask_resize_nearest_pad: Sh * Sw < 2^31 (the pixel counts are int32)");
    hipLaunchKernelGGL(mask_resize_nearest_pad_kernel, dim3(Sh, R), dim3(256), 0, (hipStream_t)stream, in, h, w, row_tab, col_tab, Sh, Sw, out, row_cnt,
                       total_zeroed);
    PSALM_LAUNCH_END("psalm_mask_resize_nearest_pad");
}

// ---------------------------------------------------------------- the idx-th set pixels of a mask, as (y / Sh, x / Sw)
// idx (R, n): ranks in row-major order of the set pixels -- row k of mask.nonzero().  Block = one mask: exclusive prefix of its per-row counts in
// LDS, then per point a binary search for the row and a walk along that row to the k-th set pixel.  A rank outside [0, set pixels) gives (0, 0).
// The quotient is the correctly rounded fp32 division of two integers below 2^24: what torch's int64 / int64 (both converted to float32) gives.
#define VIDEO_MAX_ROWS 8192
__device__ __forceinline__ float video_div(float a, float b) {
#ifdef PSALM_EMU_BUILD
    return a / b;                                                      // host build: IEEE division
#else
    return __fdiv_rn(a, b);
#endif
}
__global__ void __launch_bounds__(256) mask_select_points_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ row_cnt,
                                                                 const int* __restrict__ idx, int Sh, int Sw, int n, float* __restrict__ pts) {
    __shared__ int pre[VIDEO_MAX_ROWS + 1];                            // pre[y] = set pixels in rows < y
    __shared__ int part[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int* rc = row_cnt + (long)r * Sh;
    const int per = (Sh + 255) / 256, y0 = tid * per, y1 = min(Sh, y0 + per);
    int s = 0;
    for (int y = y0; y < y1; ++y) s += rc[y];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        pre[Sh] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int y = y0; y < y1; ++y) { pre[y] = run; run += rc[y]; }
    __syncthreads();
    const int total = pre[Sh];
    for (int i = tid; i < n; i += 256) {
        const int k = idx[(long)r * n + i];
        float py = 0.f, px = 0.f;
        if (k >= 0 && k < total) {
            int lo = 0, hi = Sh - 1;                                   // the row y with pre[y] <= k < pre[y + 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pre[mid + 1] > k) hi = mid; else lo = mid + 1;
            }
            const unsigned char* row = masks + ((long)r * Sh + lo) * Sw;
            int left = k - pre[lo], x = 0;
            for (; x < Sw; ++x)
                if (row[x] != 0 && left-- == 0) break;
            if (x < Sw) {
                py = video_div((float)lo, (float)Sh);
                px = video_div((float)x, (float)Sw);
            }
        }
        pts[((long)r * n + i) * 2] = py;
        pts[((long)r * n + i) * 2 + 1] = px;
    }
}
extern "C" int psalm_mask_select_points(const unsigned char* masks, const int* row_cnt, const int* idx, int R, int Sh, int Sw, int n, float* pts,
                                        void* stream) {
    if (R == 0 || n == 0) return 0;
    PSALM_CHECK_ARG(R >= 1 && n >= 1 && Sh >= 1 && Sh <= VIDEO_MAX_ROWS && Sw >= 1, "psalm_mask_select_points: 1 <= Sh <= 8192, Sw >= 1");
    PSALM_CHECK_ARG(Sh < (1 << 24) && Sw < (1 << 24) && (long)Sh * Sw <= INT_MAX, "psalm_mask_select_points: coordinates must be exact in float32");
    hipLaunchKernelGGL(mask_select_points_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, masks, row_cnt, idx, Sh, Sw, n, pts);
    PSALM_LAUNCH_END("psalm_mask_select_points");
}
