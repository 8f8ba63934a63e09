// Where a mask is and how large it is, on the device (psalm_amd/evalout.py mask_boxes / label_boxes): what the reference declines to compute
// because it is slow on the host -- `# result.pred_boxes = BitMasks(mask_pred > 0).get_bounding_boxes()`, psalm/model/language_model/
// llava_phi.py:319,395,438-440 -- as one bandwidth-bound pass over masks that are on the device already:
//   psalm_mask_boxes    binary masks (n,H,W) f32 | u8 -> boxes (m,4) f32 = (x_min, y_min, x_max + 1, y_max + 1) over the set pixels (detectron2
//                       BitMasks.get_bounding_boxes; an empty mask gives (0,0,0,0)) and areas (m) i32 = set pixels; an optional index list
//                       names the planes (the picked queries of a session) so that no gather copy is made
//   psalm_label_boxes   label map (H,W) i32 | u8 -> table (n_ids,5) i32 = [x0, y0, x1, y1, area] per label value (a panoptic id map, the
//                       tracker's fused map)
// All integer work, combined with integer max / add atomics only: the result does not depend on the order the blocks arrive in, so two calls
// give the same bytes (tests/test_28_mask_boxes_kernels.py).
//
// The accumulated quantities are max(W - x), max(H - y), max(x + 1), max(y + 1) and the pixel count: all are >= 1 once a pixel is set, so an
// ALL-ZERO accumulator means "empty" and one memset node initialises it; a small finishing kernel turns them into the box.
#include "common.h"

#include <climits>

#define MB_ROWS 16                  // rows of a plane per block (4 per wavefront)

template <typename T> __device__ __forceinline__ bool mb_set(T v);
template <> __device__ __forceinline__ bool mb_set<float>(float v) { return v > 0.f; }               // NaN, -0.0, negatives: not set
template <> __device__ __forceinline__ bool mb_set<unsigned char>(unsigned char v) { return v != 0; }

// the V = 16 / sizeof(T) elements of one aligned 16-byte word -> bit k = element k is set
__device__ __forceinline__ unsigned mb_word_bits(const float* p) {
    const psalm_f32x4 a = *reinterpret_cast<const psalm_f32x4*>(p);
    return (a.x > 0.f ? 1u : 0u) | (a.y > 0.f ? 2u : 0u) | (a.z > 0.f ? 4u : 0u) | (a.w > 0.f ? 8u : 0u);
}
__device__ __forceinline__ unsigned mb_word_bits(const unsigned char* p) {
    const psalm_u32x4 a = *reinterpret_cast<const psalm_u32x4*>(p);
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) bits |= ((w[i] >> (8 * k)) & 0xffu) ? 1u << (4 * i + k) : 0u;
    return bits;
}

// grid (row groups, m output rows), block = 4 wavefronts.  A wavefront walks one row at a time in steps of 64 lanes x V elements; the walk
// starts at the 16-byte boundary at or before the row's first element, so every lane's word is aligned whatever W and the plane base are:
// lanes whose word lies inside the row take one 16-byte load, the one or two lanes that straddle a row end read their elements singly.
// The lanes' "any element set" becomes a ballot word: non-zero = the row is hit, its first / last set lane (and that lane's own bit word)
// give the column extent; the pixel count is the per-lane popcount, summed over the wavefront once at the end.
template <typename T>
__global__ void __launch_bounds__(256) mask_boxes_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, int H, int W,
                                                         int* __restrict__ acc) {
    constexpr int V = 16 / (int)sizeof(T);
    __shared__ int part[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y;
    const int plane = index ? index[row] : row;
    if ((unsigned)plane >= (unsigned)n) return;                        // block-uniform: the zeroed accumulator row stays "empty"
    if (tid < 5) part[tid] = 0;
    __syncthreads();
    const T* base = masks + (long)plane * H * W;
    int xlo = INT_MAX, xhi = -1, ylo = INT_MAX, yhi = -1, cnt = 0;     // xlo .. yhi: wave-uniform; cnt: per lane
    const int y_end = min(H, ((int)blockIdx.x + 1) * MB_ROWS);
    for (int y = blockIdx.x * MB_ROWS + wave; y < y_end; y += 4) {
        const T* p = base + (long)y * W;
        const int lead = (int)(((uintptr_t)p / sizeof(T)) & (uintptr_t)(V - 1));          // elements between the 16-byte boundary and p
        for (int x0 = -lead; x0 < W; x0 += 64 * V) {                   // wave-uniform trip count
            const int x = x0 + V * lane;
            unsigned bits = 0;
            if (x >= 0 && x + V <= W) bits = mb_word_bits(p + x);
            else {
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (x + k >= 0 && x + k < W && mb_set<T>(p[x + k])) bits |= 1u << k;
            }
            cnt += __builtin_popcount(bits);
            const unsigned long long any = __ballot(bits != 0 ? 1 : 0);
            if (any) {                                                 // wave-uniform
                const int lf = __builtin_ctzll(any), ll = 63 - __builtin_clzll(any);
                const unsigned bf = __shfl(bits, lf), bl = __shfl(bits, ll);
                xlo = min(xlo, x0 + V * lf + __builtin_ctz(bf));
                xhi = max(xhi, x0 + V * ll + 31 - __builtin_clz(bl));
                ylo = min(ylo, y);
                yhi = y;                                               // rows ascend
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0 && cnt) {
        atomicMax(&part[0], W - xlo);
        atomicMax(&part[1], H - ylo);
        atomicMax(&part[2], xhi + 1);
        atomicMax(&part[3], yhi + 1);
        atomicAdd(&part[4], cnt);
    }
    __syncthreads();
    if (tid < 5 && part[4]) {                                          // one group of integer atomics per (block, plane)
        if (tid < 4) atomicMax(&acc[row * 5 + tid], part[tid]);
        else atomicAdd(&acc[row * 5 + 4], part[4]);
    }
}
__global__ void __launch_bounds__(256) mask_boxes_finish_kernel(const int* __restrict__ acc, int m, int H, int W, float* __restrict__ boxes,
                                                                int* __restrict__ areas) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int* a = acc + i * 5;
    const bool some = a[4] > 0;
    boxes[i * 4] = some ? (float)(W - a[0]) : 0.f;                     // coordinates <= 2^24: exact in float32
    boxes[i * 4 + 1] = some ? (float)(H - a[1]) : 0.f;
    boxes[i * 4 + 2] = some ? (float)a[2] : 0.f;
    boxes[i * 4 + 3] = some ? (float)a[3] : 0.f;
    areas[i] = a[4];
}
extern "C" long psalm_mask_boxes_workspace(int m) {
    return (m >= 0 && m <= 65535) ? (long)m * 5 * 4 : -1;
}
extern "C" int psalm_mask_boxes(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, float* boxes, int* areas,
                                void* workspace, long workspace_bytes, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0 && H >= 0 && W >= 0, "psalm_mask_boxes: n, m, H, W >= 0");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_boxes: without an index list the outputs have n rows (m == n)");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_boxes: at most 65535 output rows");
    PSALM_CHECK_ARG((long)H * W <= INT_MAX && H <= (1 << 24) && W <= (1 << 24),
                    "psalm_mask_boxes: H * W < 2^31 (the areas are int32), H, W <= 2^24 (the coordinates are exact in float32)");
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_mask_boxes_workspace(m) && ((uintptr_t)workspace & 3) == 0,
                    "psalm_mask_boxes: workspace of psalm_mask_boxes_workspace(m) bytes, 4-byte aligned");
    PSALM_CHECK_ARG(dtype_is_u8 || ((uintptr_t)masks & 3) == 0, "psalm_mask_boxes: float32 masks must be 4-byte aligned");
    int* acc = (int*)workspace;
    if (hipMemsetAsync(acc, 0, (size_t)m * 5 * 4, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_mask_boxes: hipMemsetAsync failed");
        return -2;
    }
    if (n > 0 && H > 0 && W > 0) {
        const dim3 grid(cdiv(H, MB_ROWS), m);
        if (dtype_is_u8) hipLaunchKernelGGL((mask_boxes_kernel<unsigned char>), grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)masks, index, n, H, W, acc);
        else hipLaunchKernelGGL((mask_boxes_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)masks, index, n, H, W, acc);
    }
    hipLaunchKernelGGL(mask_boxes_finish_kernel, dim3(cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, (const int*)acc, m, H, W, boxes, areas);
    PSALM_LAUNCH_END("psalm_mask_boxes");
}

// ---------------------------------------------------------------- boxes and areas per label value
// A wavefront takes 64 consecutive pixels of a row.  The lanes that hold the same label value as the first unserved lane form a ballot word:
// its first / last bit and popcount are that value's column extent and pixel count in the segment (a segment inside one object costs ONE
// round), and lanes 0..4 send the five quantities to the block's LDS table with LDS atomics.  The block flushes the rows it touched with
// global integer atomics into `table` itself (zeroed by the entry), which the finishing kernel rewrites in place.
#define LB_MAX_IDS 256
template <typename T>
__global__ void __launch_bounds__(256) label_boxes_kernel(const T* __restrict__ labels, int H, int W, int n_ids, int* __restrict__ table) {
    __shared__ int tab[LB_MAX_IDS * 5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < n_ids * 5; i += 256) tab[i] = 0;
    __syncthreads();
    for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
        const T* p = labels + (long)y * W;
        for (int x0 = 0; x0 < W; x0 += 64) {                           // wave-uniform trip count
            const int x = x0 + lane;
            int v = -1;
            if (x < W) {
                const long long l = (long long)p[x];
                if (l >= 0 && l < n_ids) v = (int)l;                   // values outside [0, n_ids) are ignored
            }
            unsigned long long rem = __ballot(v >= 0 ? 1 : 0);
            while (rem) {                                              // wave-uniform
                const int id = __shfl(v, __builtin_ctzll(rem));
                const unsigned long long b = __ballot(v == id ? 1 : 0);
                const int lo = x0 + __builtin_ctzll(b), hi = x0 + 63 - __builtin_clzll(b);
                const int q = lane == 0 ? W - lo : lane == 1 ? H - y : lane == 2 ? hi + 1 : lane == 3 ? y + 1 : __builtin_popcountll(b);
                if (lane < 4) atomicMax(&tab[id * 5 + lane], q);
                else if (lane == 4) atomicAdd(&tab[id * 5 + 4], q);
                rem &= ~b;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n_ids * 5; i += 256) {
        const int q = tab[i];
        if (q == 0) continue;
        if (i % 5 < 4) atomicMax(&table[i], q);
        else atomicAdd(&table[i], q);
    }
}
__global__ void __launch_bounds__(256) label_boxes_finish_kernel(int* __restrict__ table, int n_ids, int H, int W) {
    const int i = threadIdx.x;
    if (i >= n_ids) return;
    int* t = table + i * 5;
    if (t[4] > 0) {
        t[0] = W - t[0];
        t[1] = H - t[1];
    }
}
extern "C" int psalm_label_boxes(const void* labels, int dtype_is_u8, int H, int W, int n_ids, int* table, void* stream) {
    PSALM_CHECK_ARG(n_ids >= 1 && n_ids <= LB_MAX_IDS, "psalm_label_boxes: 1 <= n_ids <= 256");
    PSALM_CHECK_ARG(H >= 0 && W >= 0 && (long)H * W <= INT_MAX, "psalm_label_boxes: H, W >= 0, H * W < 2^31 (the areas are int32)");
    PSALM_CHECK_ARG(table != nullptr && ((uintptr_t)table & 3) == 0 && (dtype_is_u8 || ((uintptr_t)labels & 3) == 0),
                    "psalm_label_boxes: int32 table / labels must be 4-byte aligned");
    if (hipMemsetAsync(table, 0, (size_t)n_ids * 5 * 4, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_label_boxes: hipMemsetAsync failed");
        return -2;
    }
    if (H == 0 || W == 0) return 0;
    const int gx = cdiv(H, 4 * 4);                                     // >= 4 rows per wavefront: the LDS table is set up and flushed once per 16 rows
    if (dtype_is_u8) hipLaunchKernelGGL((label_boxes_kernel<unsigned char>), dim3(gx > 1024 ? 1024 : gx), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)labels, H, W, n_ids, table);
    else hipLaunchKernelGGL((label_boxes_kernel<int>), dim3(gx > 1024 ? 1024 : gx), dim3(256), 0, (hipStream_t)stream, (const int*)labels, H, W, n_ids, table);
    hipLaunchKernelGGL(label_boxes_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, table, n_ids, H, W);
    PSALM_LAUNCH_END("psalm_label_boxes");
}
