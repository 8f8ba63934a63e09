// Exact squared Euclidean distance maps of binary planes on the device, and what hangs on them (psalm_amd/evalout.py mask_distance / mask_centers /
// mask_boundaries / boundary_counts, PSALM.segment_everything(centers=True)): "how far is each pixel from the mask's edge".
//   psalm_mask_distance     masks (n,H,W) f32 | u8 (+ an index list naming the planes) -> dist2 (m,H,W) i32: the squared distance to the nearest seed
//                           pixel (seeds: the unset or the set pixels, optionally every position outside the image); DT_FAR where there is no seed
//   psalm_mask_centers      the same planes and their inside map -> (m,3) i32 = [y, x, dist2] of the set pixel deepest inside
//   psalm_mask_boundaries   the same planes -> (m,H,W) bytes of 0 / 1: the boundary map of DAVIS seg2bmap at the plane's own size
//   psalm_boundary_counts   prediction / target planes and a pair list -> (P,4) i64 = [n_fg, n_gt, fg_match, gt_match], the integers of DAVIS's F
// All integer work, exact: the transform is the separable one of Saito-Toriwaki / Meijster.
//
// Separate launches, no block ever waits for another or reads what another block of the same launch writes:
//   1 dt_row_kernel     a wavefront per plane row.  The set test once per pixel; 64 pixels become one ballot word, lane l of the wave keeps word
//                       64 c + l of the row.  The column of the last seed in front of a word and of the first seed behind it are an exclusive
//                       prefix max / suffix min over the lanes (six shuffles each, a carry across the groups of 64 words); inside a word the nearest
//                       seed to the left / right of a lane is a leading / trailing zero count of the masked word.  g = the distance along the row,
//                       uint16, DT_NONE for a row without a seed.  The border enters as two virtual seeds at x = -1 and x = W.
//   2 dt_col_kernel     a lane per column, a wavefront per 64 adjacent columns.  Downwards: the lower envelope of the parabolas (y - i)^2 + g[i]^2
//                       of the column, kept as a stack of (parabola, first row it owns) in the workspace, laid out [depth][column]; a parabola is
//                       pushed once and popped at most once, so the work per column is O(H) whatever the mask holds.  Sep() is Meijster's integer
//                       division.  Rows whose g is DT_NONE give no parabola; the vertical border is two virtual parabolas at y = -1 and y = H.
//                       Upwards: the envelope is read off.  A lane touches only its own column of g, of the stacks and of the output.
//   3 dt_center_kernel  a block per 2048 pixels: key = (dist2 << 32) | (0xFFFFFFFF - flat index) over the set pixels, a block maximum, ONE 64-bit
//                       atomicMax per block into the plane's slot (the key decides, not the order of arrival); dt_center_decode_kernel unpacks it
//   4 dt_boundary_kernel  a thread per pixel: m ^ e | m ^ s | m ^ se with seg2bmap's last row / column rules
//   5 dt_count_kernel   a block per 2048 pixels of a pair: four integer sums, a shuffle reduction, one atomicAdd per block and counter
#include "common.h"

#include <climits>

#define DT_FAR (1 << 30)            // no seed anywhere: above every true squared distance (H, W <= DT_MAX_SIDE)
#define DT_MAX_SIDE 16384
#define DT_NONE 0xFFFFu             // g of a row without a seed
#define DT_NO_SEED (1 << 20)        // column of a seed that is not there: +- this, further than any row is long
#define DT_WGROUPS 4                // groups of 64 ballot words: 64 * 64 * 4 = DT_MAX_SIDE pixels per row
#define DT_BLOCK_PIX 2048           // pixels per block of the centre, boundary and count passes

template <typename T> __device__ __forceinline__ bool dt_set(T v);
template <> __device__ __forceinline__ bool dt_set<float>(float v) { return v > 0.f; }               // NaN, -0.0, negatives: not set
template <> __device__ __forceinline__ bool dt_set<unsigned char>(unsigned char v) { return v != 0; }

// ---------------------------------------------------------------- 1: distance along the row
// grid (ceil(H / 4), m), block 256: wave `wave` of block b owns row 4 b + wave of output row blockIdx.y
template <typename T>
__global__ void __launch_bounds__(256) dt_row_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, int H, int W, int seeds_set,
                                                     int border, unsigned short* __restrict__ g) {
    const int lane = threadIdx.x & 63, row = blockIdx.y;
    const int y = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (y >= H) return;                                                // wave-uniform
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;                  // an invalid index is the empty plane
    const T* src = masks + ((valid ? (long)plane : 0) * H + y) * W;
    unsigned short* dst = g + ((long)row * H + y) * W;
    const int nw = (W + 63) >> 6;
    unsigned long long mine[DT_WGROUPS];                               // lane l: the seed word 64 c + l of the row (bit b: pixel 64 (64 c + l) + b)
#pragma unroll
    for (int c = 0; c < DT_WGROUPS; ++c) {
        mine[c] = 0;
        const int k1 = min(64, nw - 64 * c);                           // uniform; <= 0: the row ends in front of this group
        for (int k = 0; k < k1; ++k) {
            const int x = (64 * c + k) * 64 + lane;
            const bool seed = x < W && ((valid && dt_set<T>(src[x])) == (seeds_set != 0));
            const unsigned long long word = __ballot(seed ? 1 : 0);
            if (lane == k) mine[c] = word;
        }
    }
    // per word: the column of the last seed in the words in front of it (prefix max) and of the first seed in the words behind it (suffix min)
    int last[DT_WGROUPS], next[DT_WGROUPS];
    int carry = border ? -1 : -DT_NO_SEED;
#pragma unroll
    for (int c = 0; c < DT_WGROUPS; ++c) {
        const int w0 = (64 * c + lane) * 64;
        int v = mine[c] ? w0 + 63 - __builtin_clzll(mine[c]) : -DT_NO_SEED;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o);
            if (lane >= o) v = max(v, u);
        }
        const int ex = __shfl_up(v, 1);
        last[c] = lane ? max(ex, carry) : carry;
        carry = max(carry, __shfl(v, 63));
    }
    carry = border ? W : DT_NO_SEED;
#pragma unroll
    for (int c = DT_WGROUPS - 1; c >= 0; --c) {
        const int w0 = (64 * c + lane) * 64;
        int v = mine[c] ? w0 + __builtin_ctzll(mine[c]) : DT_NO_SEED;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_down(v, o);
            if (lane + o < 64) v = min(v, u);
        }
        const int ex = __shfl_down(v, 1);
        next[c] = lane < 63 ? min(ex, carry) : carry;
        carry = min(carry, __shfl(v, 0));
    }
    const unsigned long long upto = ~0ull >> (63 - lane), from = ~0ull << lane;      // bits 0 .. lane, bits lane .. 63
#pragma unroll
    for (int c = 0; c < DT_WGROUPS; ++c) {
        const int k1 = min(64, nw - 64 * c);
        for (int k = 0; k < k1; ++k) {
            const unsigned long long word = __shfl(mine[c], k);
            const int before = __shfl(last[c], k), behind = __shfl(next[c], k);
            const int w0 = (64 * c + k) * 64, x = w0 + lane;
            const unsigned long long lo = word & upto, hi = word & from;
            const int l = lo ? w0 + 63 - __builtin_clzll(lo) : before;
            const int r = hi ? w0 + __builtin_ctzll(hi) : behind;
            const int d = min(x - l, r - x);
            if (x < W) dst[x] = (unsigned short)(d > DT_MAX_SIDE ? DT_NONE : d);
        }
    }
}

// ---------------------------------------------------------------- 2: the lower envelope down the column
// grid (ceil(W / 64), m), block 64.  Rows are counted from 1 (i = y + 1), so that the virtual border seeds sit at i = 0 and i = H + 1 and every
// term of Sep() is non-negative.  st_s / st_t: (m, H + 2, W) uint16, entry q of column x at [q][x]: the parabola's row and the first row it owns.
// The top of the stack is mirrored in registers (cs, ct and cg = g of row cs).  Output: dist2 (m,H,W) i32, or, when `near` is given instead,
// near (m,H,W) bytes = dist2 <= thr2.
__global__ void __launch_bounds__(64) dt_col_kernel(const unsigned short* __restrict__ g, unsigned short* __restrict__ st_s, unsigned short* __restrict__ st_t,
                                                    int H, int W, int border, int* __restrict__ dist2, unsigned char* __restrict__ near, int thr2) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, row = blockIdx.y;
    if (x >= W) return;
    const unsigned short* gp = g + (long)row * H * W + x;
    unsigned short* sp = st_s + (long)row * (H + 2) * W + x;
    unsigned short* tp = st_t + (long)row * (H + 2) * W + x;
    int q = -1, cs = 0, ct = 0, cg = 0;
    const int i0 = border ? 0 : 1, i1 = border ? H + 1 : H;
    for (int i = i0; i <= i1; ++i) {
        int gi = 0;
        if (i >= 1 && i <= H) {
            gi = gp[(long)(i - 1) * W];
            if (gi == (int)DT_NONE) continue;                          // no seed in this row: no parabola
        }
        const int fi = gi * gi;
        while (q >= 0) {                                               // parabolas that the new one beats on the first row they own are gone for good
            const int a = ct - cs, b = ct - i;
            if (a * a + cg * cg <= b * b + fi) break;
            --q;
            if (q >= 0) {
                cs = sp[(long)q * W];
                ct = tp[(long)q * W];
                cg = (cs >= 1 && cs <= H) ? gp[(long)(cs - 1) * W] : 0;
            }
        }
        if (q < 0) {
            q = 0, cs = i, ct = 1, cg = gi;
            sp[0] = (unsigned short)i;
            tp[0] = 1;
        } else {
            const int w = 1 + (i * i - cs * cs + fi - cg * cg) / (2 * (i - cs));      // Sep(cs, i) + 1: the first row where i is strictly better
            if (w <= H) {
                ++q, cs = i, ct = w, cg = gi;
                sp[(long)q * W] = (unsigned short)i;
                tp[(long)q * W] = (unsigned short)w;
            }
        }
    }
    const long out = (long)row * H * W + x;
    for (int i = H; i >= 1; --i) {
        int d = DT_FAR;
        if (q >= 0) {
            const int a = i - cs;
            d = a * a + cg * cg;
            if (i == ct && q > 0) {
                --q;
                cs = sp[(long)q * W];
                ct = tp[(long)q * W];
                cg = (cs >= 1 && cs <= H) ? gp[(long)(cs - 1) * W] : 0;
            }
        }
        if (near) near[out + (long)(i - 1) * W] = d <= thr2 ? 1 : 0;
        else dist2[out + (long)(i - 1) * W] = d;
    }
}

// ---------------------------------------------------------------- 3: the pixel deepest inside
// grid (ceil(HW / DT_BLOCK_PIX), m), block 256; slots (m) u64, zeroed
template <typename T>
__global__ void __launch_bounds__(256) dt_center_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, long HW,
                                                        const int* __restrict__ dist2, unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long s_key[4];
    const int tid = threadIdx.x, row = blockIdx.y;
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;
    const T* base = masks + (valid ? (long)plane * HW : 0);
    unsigned long long key = 0;
#pragma unroll
    for (int j = 0; j < DT_BLOCK_PIX / 256; ++j) {
        const long p = (long)blockIdx.x * DT_BLOCK_PIX + 256 * j + tid;
        if (p < HW && valid && dt_set<T>(base[p])) {
            const unsigned long long k = ((unsigned long long)(unsigned)dist2[(long)row * HW + p] << 32) | (0xFFFFFFFFull - (unsigned long long)p);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(key, o);
        key = u > key ? u : key;
    }
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) key = s_key[k] > key ? s_key[k] : key;
        if (key) atomicMax(&slots[row], key);
    }
}
// grid (ceil(m / 256)): centers (m,3) i32 = [y, x, dist2], [-1, -1, 0] for a plane without a set pixel
__global__ void __launch_bounds__(256) dt_center_decode_kernel(const unsigned long long* __restrict__ slots, int m, int W, int* __restrict__ centers) {
    const int row = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (row >= m) return;
    const unsigned long long key = slots[row];
    int y = -1, x = -1, d = 0;
    if (key) {
        const unsigned p = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        y = (int)(p / (unsigned)W), x = (int)(p % (unsigned)W), d = (int)(key >> 32);
    }
    centers[3 * row] = y;
    centers[3 * row + 1] = x;
    centers[3 * row + 2] = d;
}

// ---------------------------------------------------------------- 4: boundary maps
// grid (ceil(HW / DT_BLOCK_PIX), m), block 256
template <typename T>
__global__ void __launch_bounds__(256) dt_boundary_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, int H, int W,
                                                          unsigned char* __restrict__ out) {
    const int tid = threadIdx.x, row = blockIdx.y;
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;
    const long HW = (long)H * W;
    const T* base = masks + (valid ? (long)plane * HW : 0);
#pragma unroll
    for (int j = 0; j < DT_BLOCK_PIX / 256; ++j) {
        const long p = (long)blockIdx.x * DT_BLOCK_PIX + 256 * j + tid;
        if (p >= HW) break;
        const int y = (int)(p / W), x = (int)(p % W);
        const bool right = x + 1 < W, below = y + 1 < H;
        unsigned char b = 0;
        if (valid) {
            const bool m = dt_set<T>(base[p]);
            const bool e = right && dt_set<T>(base[p + 1]), s = below && dt_set<T>(base[p + W]), se = right && below && dt_set<T>(base[p + W + 1]);
            if (right && below) b = (m != e) || (m != s) || (m != se);
            else if (right) b = m != e;                                // the last row
            else if (below) b = m != s;                                // the last column; the last pixel stays 0
        }
        out[(long)row * HW + p] = b;
    }
}

// ---------------------------------------------------------------- 5: boundary counts of a pair list
// grid (ceil(HW / DT_BLOCK_PIX), P), block 256.  bmap / near (M,HW) bytes of 0 / 1: rows [0, mp) the predictions, [mp, mp + mt) the targets.
// counts (P,4) u64, zeroed: [n_fg, n_gt, fg_match, gt_match]; a pair with an index outside its list adds nothing.
__global__ void __launch_bounds__(256) dt_count_kernel(const unsigned char* __restrict__ bmap, const unsigned char* __restrict__ near,
                                                       const int* __restrict__ pair_p, const int* __restrict__ pair_t, int mp, int mt, long HW,
                                                       unsigned long long* __restrict__ counts) {
    __shared__ int s_cnt[4][4];
    const int tid = threadIdx.x, pair = blockIdx.y;
    const int a = pair_p[pair], b = pair_t[pair];
    if ((unsigned)a >= (unsigned)mp || (unsigned)b >= (unsigned)mt) return;            // block-uniform
    const unsigned char *ba = bmap + (long)a * HW, *bb = bmap + (long)(mp + b) * HW;
    const unsigned char *na = near + (long)a * HW, *nb = near + (long)(mp + b) * HW;
    int c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < DT_BLOCK_PIX / 256; ++j) {
        const long p = (long)blockIdx.x * DT_BLOCK_PIX + 256 * j + tid;
        if (p >= HW) break;
        const int fa = ba[p], fb = bb[p];
        c[0] += fa;
        c[1] += fb;
        c[2] += fa & nb[p];
        c[3] += fb & na[p];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o);
        if ((tid & 63) == 0) s_cnt[tid >> 6][k] = c[k];
    }
    __syncthreads();
    if (tid < 4) {
        const int v = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        if (v) atomicAdd(&counts[4 * (long)pair + tid], (unsigned long long)v);
    }
}

// ---------------------------------------------------------------- entries
static long dt_align(long v) { return (v + 255) / 256 * 256; }
static bool dt_dims_ok(int m, int H, int W) { return m >= 0 && m <= 65535 && H >= 1 && H <= DT_MAX_SIDE && W >= 1 && W <= DT_MAX_SIDE; }
// g (m,H,W) u16 | the two stacks (m,H + 2,W) u16 each
static long dt_g_bytes(int m, int H, int W) { return dt_align((long)m * H * W * 2); }
static long dt_stack_bytes(int m, int H, int W) { return dt_align((long)m * (H + 2) * W * 2); }

extern "C" long psalm_mask_distance_workspace(int m, int H, int W) {
    if (!dt_dims_ok(m, H, W)) return -1;
    return dt_g_bytes(m, H, W) + 2 * dt_stack_bytes(m, H, W);
}

// the two passes on m planes; exactly one of dist2 / near is given
template <typename T>
static void dt_run(const T* masks, const int* index, int n, int H, int W, int m, int seeds_set, int border, int* dist2, unsigned char* near, int thr2,
                   char* ws, hipStream_t s) {
    unsigned short* g = (unsigned short*)ws;
    unsigned short* st_s = (unsigned short*)(ws + dt_g_bytes(m, H, W));
    unsigned short* st_t = (unsigned short*)(ws + dt_g_bytes(m, H, W) + dt_stack_bytes(m, H, W));
    hipLaunchKernelGGL((dt_row_kernel<T>), dim3(cdiv(H, 4), m), dim3(256), 0, s, masks, index, n, H, W, seeds_set, border, g);
    hipLaunchKernelGGL(dt_col_kernel, dim3(cdiv(W, 64), m), dim3(64), 0, s, (const unsigned short*)g, st_s, st_t, H, W, border, dist2, near, thr2);
}

extern "C" int psalm_mask_distance(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, int to_set, int border, int* dist2,
                                   void* workspace, long workspace_bytes, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0, "psalm_mask_distance: n, m >= 0");
    PSALM_CHECK_ARG(H >= 1 && H <= DT_MAX_SIDE && W >= 1 && W <= DT_MAX_SIDE, "psalm_mask_distance: 1 <= H, W <= 16384");
    PSALM_CHECK_ARG(to_set == 0 || to_set == 1, "psalm_mask_distance: to_set is 0 (distance to the unset pixels) or 1 (to the set pixels)");
    PSALM_CHECK_ARG(border == 0 || border == 1, "psalm_mask_distance: border is 0 or 1");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_distance: without an index list the outputs have n rows (m == n)");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_distance: at most 65535 output rows");
    PSALM_CHECK_ARG(dist2 != nullptr && ((uintptr_t)dist2 & 3) == 0, "psalm_mask_distance: dist2 must be 4-byte aligned");
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_mask_distance_workspace(m, H, W) && ((uintptr_t)workspace & 255) == 0,
                    "psalm_mask_distance: workspace of psalm_mask_distance_workspace(m, H, W) bytes, 256-byte aligned");
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_distance: float32 masks must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype_is_u8) dt_run((const unsigned char*)masks, index, n, H, W, m, to_set, border, dist2, nullptr, 0, (char*)workspace, s);
    else dt_run((const float*)masks, index, n, H, W, m, to_set, border, dist2, nullptr, 0, (char*)workspace, s);
    PSALM_LAUNCH_END("psalm_mask_distance");
}

extern "C" int psalm_mask_centers(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, const int* dist2,
                                  unsigned long long* slots, int* centers, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0, "psalm_mask_centers: n, m >= 0");
    PSALM_CHECK_ARG(H >= 1 && H <= DT_MAX_SIDE && W >= 1 && W <= DT_MAX_SIDE, "psalm_mask_centers: 1 <= H, W <= 16384");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_centers: without an index list the outputs have n rows (m == n)");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_centers: at most 65535 output rows");
    PSALM_CHECK_ARG(dist2 != nullptr && centers != nullptr && (((uintptr_t)dist2 | (uintptr_t)centers) & 3) == 0,
                    "psalm_mask_centers: dist2 / centers must be 4-byte aligned");
    PSALM_CHECK_ARG(slots != nullptr && ((uintptr_t)slots & 7) == 0, "psalm_mask_centers: slots (m 64-bit words) must be 8-byte aligned");
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_centers: float32 masks must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(slots, 0, (size_t)m * 8, s) != hipSuccess) {
        psalm_set_error("psalm_mask_centers: hipMemsetAsync failed");
        return -2;
    }
    const long HW = (long)H * W;
    const dim3 grid(cdiv(HW, DT_BLOCK_PIX), m);
    if (dtype_is_u8) hipLaunchKernelGGL((dt_center_kernel<unsigned char>), grid, dim3(256), 0, s, (const unsigned char*)masks, index, n, HW, dist2, slots);
    else hipLaunchKernelGGL((dt_center_kernel<float>), grid, dim3(256), 0, s, (const float*)masks, index, n, HW, dist2, slots);
    hipLaunchKernelGGL(dt_center_decode_kernel, dim3(cdiv(m, 256)), dim3(256), 0, s, (const unsigned long long*)slots, m, W, centers);
    PSALM_LAUNCH_END("psalm_mask_centers");
}

template <typename T>
static void dt_boundaries(const T* masks, const int* index, int n, int H, int W, int m, unsigned char* out, hipStream_t s) {
    hipLaunchKernelGGL((dt_boundary_kernel<T>), dim3(cdiv((long)H * W, DT_BLOCK_PIX), m), dim3(256), 0, s, masks, index, n, H, W, out);
}

extern "C" int psalm_mask_boundaries(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, unsigned char* out, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0, "psalm_mask_boundaries: n, m >= 0");
    PSALM_CHECK_ARG(H >= 1 && H <= DT_MAX_SIDE && W >= 1 && W <= DT_MAX_SIDE, "psalm_mask_boundaries: 1 <= H, W <= 16384");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_boundaries: without an index list the outputs have n rows (m == n)");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_boundaries: at most 65535 output rows");
    PSALM_CHECK_ARG(out != nullptr, "psalm_mask_boundaries: out is NULL");
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_boundaries: float32 masks must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype_is_u8) dt_boundaries((const unsigned char*)masks, index, n, H, W, m, out, s);
    else dt_boundaries((const float*)masks, index, n, H, W, m, out, s);
    PSALM_LAUNCH_END("psalm_mask_boundaries");
}

// the distance passes of psalm_boundary_counts run on at most this many planes at a time, through one piece of workspace
static int dt_count_chunk(int M, int H, int W) {
    const long per = psalm_mask_distance_workspace(1, H, W);
    return (int)max(1L, min((long)M, (64L << 20) / per));
}

extern "C" long psalm_boundary_counts_workspace(int mp, int mt, int H, int W) {
    if (mp < 0 || mt < 0 || !dt_dims_ok(mp + mt, H, W)) return -1;
    const int M = mp + mt;
    if (M == 0) return 0;
    return 2 * dt_align((long)M * H * W) + psalm_mask_distance_workspace(dt_count_chunk(M, H, W), H, W);      // boundary maps | near maps | the passes' own
}

extern "C" int psalm_boundary_counts(const void* pred, int pred_is_u8, int n_pred, const int* pred_index, int mp, const void* gt, int gt_is_u8, int n_gt,
                                     const int* gt_index, int mt, int H, int W, const int* pair_pred, const int* pair_gt, int P, int bound,
                                     long long* counts, void* workspace, long workspace_bytes, void* stream) {
    PSALM_CHECK_ARG(n_pred >= 0 && n_gt >= 0 && mp >= 0 && mt >= 0 && P >= 0, "psalm_boundary_counts: n_pred, n_gt, mp, mt, P >= 0");
    PSALM_CHECK_ARG(H >= 1 && H <= DT_MAX_SIDE && W >= 1 && W <= DT_MAX_SIDE, "psalm_boundary_counts: 1 <= H, W <= 16384");
    PSALM_CHECK_ARG(bound >= 0 && bound <= 32767, "psalm_boundary_counts: 0 <= bound <= 32767");
    PSALM_CHECK_ARG((pred_index != nullptr || mp == n_pred) && (gt_index != nullptr || mt == n_gt),
                    "psalm_boundary_counts: without an index list the planes are all of them (mp == n_pred, mt == n_gt)");
    if (P == 0) return 0;
    PSALM_CHECK_ARG(P <= 65535 && (long)mp + mt <= 65535, "psalm_boundary_counts: at most 65535 pairs and 65535 planes");
    PSALM_CHECK_ARG(counts != nullptr && ((uintptr_t)counts & 7) == 0, "psalm_boundary_counts: counts must be 8-byte aligned");
    PSALM_CHECK_ARG(pair_pred != nullptr && pair_gt != nullptr, "psalm_boundary_counts: pair lists are NULL");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)P * 4 * 8, s) != hipSuccess) {
        psalm_set_error("psalm_boundary_counts: hipMemsetAsync failed");
        return -2;
    }
    if (mp == 0 || mt == 0) return 0;                                  // every pair names a plane that is not there
    const int M = mp + mt;
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_boundary_counts_workspace(mp, mt, H, W) && ((uintptr_t)workspace & 255) == 0,
                    "psalm_boundary_counts: workspace of psalm_boundary_counts_workspace(mp, mt, H, W) bytes, 256-byte aligned");
    PSALM_CHECK_ARG(pred != nullptr && gt != nullptr && (pred_is_u8 || ((uintptr_t)pred & 3) == 0) && (gt_is_u8 || ((uintptr_t)gt & 3) == 0),
                    "psalm_boundary_counts: float32 masks must be 4-byte aligned");
    const long HW = (long)H * W;
    unsigned char* bmap = (unsigned char*)workspace;
    unsigned char* near = bmap + dt_align((long)M * HW);
    char* ws = (char*)near + dt_align((long)M * HW);
    if (pred_is_u8) dt_boundaries((const unsigned char*)pred, pred_index, n_pred, H, W, mp, bmap, s);
    else dt_boundaries((const float*)pred, pred_index, n_pred, H, W, mp, bmap, s);
    if (gt_is_u8) dt_boundaries((const unsigned char*)gt, gt_index, n_gt, H, W, mt, bmap + (long)mp * HW, s);
    else dt_boundaries((const float*)gt, gt_index, n_gt, H, W, mt, bmap + (long)mp * HW, s);
    const int chunk = dt_count_chunk(M, H, W);
    const int thr2 = (int)min((long)bound * bound, (long)DT_FAR - 1);  // (no true squared distance reaches DT_FAR: a plane without boundary matches nothing)
    for (int r0 = 0; r0 < M; r0 += chunk) {                            // stream order lets the chunks share the passes' workspace
        const int k = min(chunk, M - r0);
        dt_run((const unsigned char*)(bmap + (long)r0 * HW), nullptr, k, H, W, k, 1, 0, nullptr, near + (long)r0 * HW, thr2, ws, s);
    }
    hipLaunchKernelGGL(dt_count_kernel, dim3(cdiv(HW, DT_BLOCK_PIX), P), dim3(256), 0, s, (const unsigned char*)bmap, (const unsigned char*)near, pair_pred,
                       pair_gt, mp, mt, HW, (unsigned long long*)counts);
    PSALM_LAUNCH_END("psalm_boundary_counts");
}
