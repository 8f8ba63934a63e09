// Connected components of binary planes on the device (psalm_amd/evalout.py mask_components / clean_masks, PSALM.segment_everything(min_island=,
// max_hole=)): the one primitive behind "drop regions below N pixels", "fill holes below N pixels" and "split a mask into its parts".
//   psalm_mask_components   masks (n,H,W) f32 | u8 (+ an index list naming the planes) -> labels (m,H,W) i32, count (m) i32 and an optional table
//                           (m,max_comp,6) i32 = [x0, y0, x1, y1, area, border] per component
//   psalm_mask_clean        the same planes -> out (m,H,W) bytes of 0 / 1 with the small holes filled and then the small islands cleared, areas /
//                           filled / removed (m) i32
// The canonical result: a component's label is 1 + its rank among the plane's components ordered by their LOWEST row-major pixel index (the
// numbering of scipy.ndimage.label).  It falls out of a union-find whose root is always the smallest index of its set: the root of a component
// IS its lowest pixel, its rank the number of roots in front of it.  All integer work; what blocks combine they combine with integer min / max /
// add atomics: exact, independent of the order of arrival.
//
// Separate launches, no block ever waits for another:
//   1 cc_tile_label_kernel   one block per CC_T x CC_T tile of one plane: the set test once per pixel, a pixel union-find in LDS (LDS atomicMin),
//                            every pixel's in-tile root written as a global flat index into the `parent` plane (-1: not of the labelled class)
//   2 cc_merge_kernel        one thread per pixel on a tile's right column / bottom row: its right, lower and (8) diagonal neighbours in the next
//                            tile are united with a lock-free loop on `parent`
//   3 cc_accumulate_kernel   one block per tile again: root = find(pixel) -- done once per in-tile set by its head, shared through LDS -- goes to a
//                            SECOND plane (the labels), never over the links being read; area and border flag are reduced per in-tile set in LDS
//                            and leave the block as ONE global atomic per set into plane-sized slot arrays at the root's index
//   4 cc_count_roots / cc_scan_blocks / cc_assign / cc_relabel    a two-level exclusive scan of "is a root" numbers the roots; the relabel pass
//                            extends the table's boxes with integer min / max atomics, one group per run of equal labels in a wavefront
// psalm_mask_clean runs 1 - 3 (without the root plane) and a decision pass per step; it needs no numbering.
//
// WHY STALE LINKS ARE HARMLESS IN LAUNCH 2 (the only launch that reads links while others lower them).  On gfx950 a plain load may be served from
// an XCD's L2 (or a CU's L1) while another XCD has already lowered that word with a device-scope atomic.  Links only ever DECREASE, and every value
// ever stored at parent[x] is a member of x's component that is <= x.  find() over stale links therefore still walks downwards inside the
// component and stops at a pixel that WAS a root; the union itself is the returning atomicMin(&parent[hi], lo): if it returns hi the link is made
// on the true root; otherwise the race is lost (or the root was stale) and the loop goes on from the value the atomic RETURNED, which is < hi, so
// every round strictly lowers hi and the loop ends.  A stale read costs iterations, never correctness.  Nothing here relies on a plain load seeing
// another block's write inside one launch; launches 3 and 4 read what earlier launches finished.
#include "common.h"

#include <climits>

#define CC_T 32                     // tile edge: CC_T x CC_T pixels per block, 4 per thread
#define CC_PIX (CC_T * CC_T)
#define CC_SCAN 1024                // pixels per block of the numbering scan, 4 consecutive ones per thread
#define CC_GATHER 2048              // pixels per block of the binarising gather

template <typename T> __device__ __forceinline__ bool cc_set(T v);
template <> __device__ __forceinline__ bool cc_set<float>(float v) { return v > 0.f; }               // NaN, -0.0, negatives: not set
template <> __device__ __forceinline__ bool cc_set<unsigned char>(unsigned char v) { return v != 0; }

// links point downwards: the walk ends at the first x with par[x] == x
__device__ __forceinline__ int cc_find(const int* par, int x) {
    for (;;) {
        const int p = par[x];
        if (p == x) return x;
        x = p;
    }
}
// unite the sets of a and b under the smaller root (see the note on stale links above)
__device__ __forceinline__ void cc_union(int* par, int a, int b) {
    for (;;) {
        a = cc_find(par, a);
        b = cc_find(par, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(&par[hi], lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// ---------------------------------------------------------------- 1: tile-local labelling
// grid (tiles, m), block 256; thread t owns the in-tile pixels t + 256 j (row (t + 256 j) / 32, column % 32)
template <typename T>
__global__ void __launch_bounds__(256) cc_tile_label_kernel(const T* __restrict__ masks, const int* __restrict__ index, int* __restrict__ parent, int n,
                                                            int H, int W, int tiles_x, int conn8, int invert) {
    __shared__ int s_par[CC_PIX];
    const int tid = threadIdx.x, row = blockIdx.y;
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;                  // block-uniform; an invalid index is the empty plane
    const long HW = (long)H * W;
    const T* base = masks + (valid ? (long)plane * HW : 0);
    int* par = parent + (long)row * HW;
    const int x0 = ((int)blockIdx.x % tiles_x) * CC_T, y0 = ((int)blockIdx.x / tiles_x) * CC_T;
    unsigned lab = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j, x = x0 + (i & (CC_T - 1)), y = y0 + i / CC_T;
        const bool in = x < W && y < H;
        const bool set = in && valid && cc_set<T>(base[(long)y * W + x]);
        const bool l = in && (set != (invert != 0));
        if (l) lab |= 1u << j;
        s_par[i] = l ? i : -1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!((lab >> j) & 1u)) continue;
        const int i = tid + 256 * j, lx = i & (CC_T - 1), ly = i / CC_T;
        if (lx > 0 && s_par[i - 1] >= 0) cc_union(s_par, i, i - 1);
        if (ly > 0) {
            if (s_par[i - CC_T] >= 0) cc_union(s_par, i, i - CC_T);
            if (conn8) {
                if (lx > 0 && s_par[i - CC_T - 1] >= 0) cc_union(s_par, i, i - CC_T - 1);
                if (lx < CC_T - 1 && s_par[i - CC_T + 1] >= 0) cc_union(s_par, i, i - CC_T + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j, x = x0 + (i & (CC_T - 1)), y = y0 + i / CC_T;
        if (x >= W || y >= H) continue;
        int p = -1;
        if ((lab >> j) & 1u) {
            const int r = cc_find(s_par, i);
            p = (y0 + r / CC_T) * W + x0 + (r & (CC_T - 1));
        }
        par[y * W + x] = p;
    }
}

// ---------------------------------------------------------------- 2: merge across tile edges
// grid (ceil(seam pixels / 256), m).  Seam pixels: first the (tiles_x - 1) H pixels of the tiles' right columns, then the (tiles_y - 1) W pixels
// of their bottom rows.  Every pair of neighbours that lies in two tiles has a seam pixel on one side (pairs that differ in the tile column are
// taken from the right column, the others from the bottom row).
__global__ void __launch_bounds__(256) cc_merge_kernel(int* __restrict__ parent, int H, int W, int tiles_x, int tiles_y, int conn8) {
    const long nv = (long)(tiles_x - 1) * H, nh = (long)(tiles_y - 1) * W;
    long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nv + nh) return;
    int* par = parent + (long)blockIdx.y * H * W;
    if (t < nv) {
        const int x = ((int)(t / H) + 1) * CC_T - 1, y = (int)(t % H), a = y * W + x;        // x + 1 < W: this is not the last tile column
        if (par[a] < 0) return;
        if (par[a + 1] >= 0) cc_union(par, a, a + 1);
        if (conn8) {
            if (y > 0 && par[a + 1 - W] >= 0) cc_union(par, a, a + 1 - W);
            if (y + 1 < H && par[a + 1 + W] >= 0) cc_union(par, a, a + 1 + W);
        }
    } else {
        t -= nv;
        const int y = ((int)(t / W) + 1) * CC_T - 1, x = (int)(t % W), a = y * W + x;        // y + 1 < H: this is not the last tile row
        if (par[a] < 0) return;
        if (par[a + W] >= 0) cc_union(par, a, a + W);
        if (conn8) {
            if (x > 0 && par[a + W - 1] >= 0) cc_union(par, a, a + W - 1);
            if (x + 1 < W && par[a + W + 1] >= 0) cc_union(par, a, a + W + 1);
        }
    }
}

// ---------------------------------------------------------------- the roots of a tile's pixels
// After launch 2 a pixel's link is its in-tile root of launch 1 (only links of such roots were ever lowered), or, for a lowered root, any smaller
// member of its component.  key = the link's in-tile index when it points into this tile, else the pixel's own: pixels with one key belong to
// one component, and the key's own pixel -- the HEAD -- does the one global find for all of them.  Leaves key[j] (-1: not labelled) and, behind a
// barrier, s_root[k] for every key k in use.  s_head[k] != 0 marks the heads.
__device__ __forceinline__ void cc_tile_roots(const int* par, int H, int W, int x0, int y0, int tid, int* s_head, int* s_root, int (&key)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s_head[tid + 256 * j] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j, x = x0 + (i & (CC_T - 1)), y = y0 + i / CC_T;
        key[j] = -1;
        if (x >= W || y >= H) continue;
        const int q = par[y * W + x];
        if (q < 0) continue;
        const int qx = q % W - x0, qy = q / W - y0;
        const int k = ((unsigned)qx < (unsigned)CC_T && (unsigned)qy < (unsigned)CC_T) ? qy * CC_T + qx : i;
        key[j] = k;
        s_head[k] = 1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j;
        if (s_head[i]) s_root[i] = cc_find(par, (y0 + i / CC_T) * W + x0 + (i & (CC_T - 1)));
    }
    __syncthreads();
}

// ---------------------------------------------------------------- 3: flatten, per-root area and border flag
// grid (tiles, m).  root_out (may be NULL): the plane that receives root[p] (-1: not labelled).  area / border: zeroed slot planes.
__global__ void __launch_bounds__(256) cc_accumulate_kernel(const int* __restrict__ parent, int* __restrict__ root_out, int* __restrict__ area,
                                                            int* __restrict__ border, int H, int W, int tiles_x) {
    __shared__ int s_head[CC_PIX], s_root[CC_PIX], s_area[CC_PIX], s_bord[CC_PIX];
    const int tid = threadIdx.x;
    const long off = (long)blockIdx.y * H * W;
    const int x0 = ((int)blockIdx.x % tiles_x) * CC_T, y0 = ((int)blockIdx.x / tiles_x) * CC_T;
#pragma unroll
    for (int j = 0; j < 4; ++j) s_area[tid + 256 * j] = s_bord[tid + 256 * j] = 0;
    int key[4];
    cc_tile_roots(parent + off, H, W, x0, y0, tid, s_head, s_root, key);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j, x = x0 + (i & (CC_T - 1)), y = y0 + i / CC_T;
        if (x >= W || y >= H) continue;
        if (key[j] >= 0) {
            atomicAdd(&s_area[key[j]], 1);
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) atomicMax(&s_bord[key[j]], 1);
        }
        if (root_out) root_out[off + y * W + x] = key[j] >= 0 ? s_root[key[j]] : -1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j;
        if (s_area[i] > 0) {                                           // a head: one group of atomics per in-tile set
            atomicAdd(&area[off + s_root[i]], s_area[i]);
            if (s_bord[i]) atomicMax(&border[off + s_root[i]], 1);
        }
    }
}

// ---------------------------------------------------------------- 4: number the roots
// exclusive scan of v over the block's 256 threads (s: 512 ints of LDS); total = the block's sum
__device__ __forceinline__ int cc_block_scan(int v, int* s, int tid, int& total) {
    int cur = 0;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        int x = s[cur * 256 + tid];
        if (tid >= o) x += s[cur * 256 + tid - o];
        s[(cur ^ 1) * 256 + tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    total = s[cur * 256 + 255];
    const int incl = s[cur * 256 + tid];
    __syncthreads();
    return incl - v;
}
// grid (nb, m): bsum[row][b] = roots among the pixels [b CC_SCAN, (b + 1) CC_SCAN)
__global__ void __launch_bounds__(256) cc_count_roots_kernel(const int* __restrict__ root, long HW, int nb, int* __restrict__ bsum) {
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const int* r = root + (long)blockIdx.y * HW;
    const long p0 = (long)blockIdx.x * CC_SCAN + 4 * tid;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p0 + k < HW && r[p0 + k] == (int)(p0 + k)) ++c;
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0) bsum[(long)blockIdx.y * nb + blockIdx.x] = s_cnt;
}
// grid (m), one block per plane: bsum[row] becomes its own exclusive scan, count[row] the number of roots
__global__ void __launch_bounds__(256) cc_scan_blocks_kernel(int* __restrict__ bsum, int nb, int* __restrict__ count) {
    __shared__ int s[512];
    const int tid = threadIdx.x;
    int* b = bsum + (long)blockIdx.x * nb;
    int carry = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {                             // block-uniform trip count
        const int v = c0 + tid < nb ? b[c0 + tid] : 0;
        int total;
        const int ex = cc_block_scan(v, s, tid, total);
        if (c0 + tid < nb) b[c0 + tid] = carry + ex;
        carry += total;
    }
    if (tid == 0) count[blockIdx.x] = carry;
}
// grid (nb, m): the root at pixel p gets its number k = 1 + rank, left in rank[p] (the dead `parent` plane), and starts its table row from
// itself: [x, y, x + 1, y + 1, area, border] -- y0 is final (the root is the component's lowest pixel), the relabel pass extends the rest
__global__ void __launch_bounds__(256) cc_assign_kernel(const int* __restrict__ root, const int* __restrict__ bsum, const int* __restrict__ area,
                                                        const int* __restrict__ border, int* __restrict__ rank, int* __restrict__ table, int H, int W,
                                                        int nb, int max_comp) {
    __shared__ int s[512];
    const int tid = threadIdx.x, row = blockIdx.y;
    const long HW = (long)H * W, off = (long)row * HW;
    const long p0 = (long)blockIdx.x * CC_SCAN + 4 * tid;
    unsigned is_root = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p0 + k < HW && root[off + p0 + k] == (int)(p0 + k)) is_root |= 1u << k;
    int total;
    int num = bsum[(long)row * nb + blockIdx.x] + cc_block_scan(__builtin_popcount(is_root), s, tid, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((is_root >> k) & 1u)) continue;
        const long p = p0 + k;
        ++num;
        rank[off + p] = num;
        if (table && num <= max_comp) {
            int* t = table + ((long)row * max_comp + num - 1) * 6;
            const int x = (int)(p % W), y = (int)(p / W);
            t[0] = x;
            t[1] = y;
            t[2] = x + 1;
            t[3] = y + 1;
            t[4] = area[off + p];
            t[5] = border[off + p];
        }
    }
}
// grid (ceil(H ceil(W / 64) / 4), m), a wavefront per 64 consecutive pixels of a row: labels[p] (holding root[p]) becomes the root's number.  The
// lanes that hold the label of the first unserved lane form a ballot word: its first / last bit is that component's column extent in the
// segment, which lanes 0 .. 2 send to the table (x0 min, x1 max, y1 max).
__global__ void __launch_bounds__(256) cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ rank, int* __restrict__ table, int H, int W,
                                                         int max_comp) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y;
    const int nseg = (W + 63) / 64;
    const long seg = (long)blockIdx.x * 4 + wave;
    if (seg >= (long)H * nseg) return;                                 // wave-uniform
    const long off = (long)row * H * W;
    const int y = (int)(seg / nseg), xs = (int)(seg % nseg) * 64, x = xs + lane;
    int k = 0;
    if (x < W) {
        const int r = labels[off + (long)y * W + x];
        k = r >= 0 ? rank[off + r] : 0;
        labels[off + (long)y * W + x] = k;
    }
    if (!table) return;                                                // uniform
    const int v = (k >= 1 && k <= max_comp) ? k : 0;
    unsigned long long rem = __ballot(v != 0 ? 1 : 0);
    while (rem) {                                                      // wave-uniform
        const int id = __shfl(v, __builtin_ctzll(rem));
        const unsigned long long b = __ballot(v == id ? 1 : 0);
        int* t = table + ((long)row * max_comp + id - 1) * 6;
        if (lane == 0) atomicMin(&t[0], xs + __builtin_ctzll(b));
        else if (lane == 1) atomicMax(&t[2], xs + 64 - __builtin_clzll(b));
        else if (lane == 2) atomicMax(&t[3], y + 1);
        rem &= ~b;
    }
}

// ---------------------------------------------------------------- cleanup passes
// grid (ceil(HW / CC_GATHER), m): out[row][p] = plane index[row] is set at p; areas[row] (zeroed) += the set pixels, one atomic per block
template <typename T>
__global__ void __launch_bounds__(256) cc_gather_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, long HW,
                                                        unsigned char* __restrict__ out, int* __restrict__ areas) {
    __shared__ int s_cnt;
    const int tid = threadIdx.x, row = blockIdx.y;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;
    const T* base = masks + (valid ? (long)plane * HW : 0);
    int c = 0;
#pragma unroll
    for (int j = 0; j < CC_GATHER / 256; ++j) {
        const long p = (long)blockIdx.x * CC_GATHER + 256 * j + tid;
        if (p >= HW) break;
        const bool set = valid && cc_set<T>(base[p]);
        out[(long)row * HW + p] = set ? 1 : 0;
        c += set ? 1 : 0;
    }
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(&areas[row], s_cnt);
}
// grid (tiles, m).  fill != 0: the labelled pixels are UNSET ones; a component that misses the image border and has at most `thresh` pixels
// becomes set.  fill == 0: the labelled pixels are set ones; a component of fewer than `thresh` pixels is cleared.  changed[row] += the pixels
// rewritten, areas[row] += / -= the same; one pair of atomics per block.
__global__ void __launch_bounds__(256) cc_decide_kernel(const int* __restrict__ parent, const int* __restrict__ area, const int* __restrict__ border,
                                                        unsigned char* __restrict__ out, int* __restrict__ changed, int* __restrict__ areas, int H, int W,
                                                        int tiles_x, int fill, int thresh) {
    __shared__ int s_head[CC_PIX], s_root[CC_PIX];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, row = blockIdx.y;
    const long off = (long)row * H * W;
    const int x0 = ((int)blockIdx.x % tiles_x) * CC_T, y0 = ((int)blockIdx.x / tiles_x) * CC_T;
    if (tid == 0) s_cnt = 0;
    int key[4];
    cc_tile_roots(parent + off, H, W, x0, y0, tid, s_head, s_root, key);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                      // a head turns its root into its component's verdict
        const int i = tid + 256 * j;
        if (s_head[i]) {
            const long r = off + s_root[i];
            s_root[i] = fill ? (border[r] == 0 && area[r] <= thresh) : (area[r] < thresh);
        }
    }
    __syncthreads();
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j;
        if (key[j] >= 0 && s_root[key[j]]) {
            out[off + (long)(y0 + i / CC_T) * W + x0 + (i & (CC_T - 1))] = fill ? 1 : 0;
            ++c;
        }
    }
    if (c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (tid == 0 && s_cnt) {
        atomicAdd(&changed[row], s_cnt);
        atomicAdd(&areas[row], fill ? s_cnt : -s_cnt);
    }
}

// ---------------------------------------------------------------- entries
static bool cc_dims_ok(int m, int H, int W) { return m >= 0 && m <= 65535 && H >= 0 && W >= 0 && (long)H * W <= INT_MAX; }
static long cc_scan_blocks(int H, int W) { return ((long)H * W + CC_SCAN - 1) / CC_SCAN; }

extern "C" long psalm_mask_components_workspace(int m, int H, int W) {
    if (!cc_dims_ok(m, H, W)) return -1;
    return (long)m * (3 * (long)H * W + cc_scan_blocks(H, W)) * 4;      // parent / rank, area, border planes + the scan's block sums
}
extern "C" long psalm_mask_clean_workspace(int m, int H, int W) {
    if (!cc_dims_ok(m, H, W)) return -1;
    return (long)m * 3 * (long)H * W * 4;                               // parent, area, border planes
}

// launches 1 - 3 on m planes; ws: parent | area | border (m HW ints each); root_out may be NULL
template <typename T>
static int cc_label(const T* masks, const int* index, int n, int m, int H, int W, int conn8, int invert, int* ws, int* root_out, hipStream_t stream,
                    const char* who) {
    const long plane = (long)m * H * W;
    int *parent = ws, *area = ws + plane, *border = ws + 2 * plane;
    if (hipMemsetAsync(area, 0, (size_t)plane * 2 * 4, stream) != hipSuccess) {
        psalm_set_error(who);
        return -2;
    }
    const int tx = cdiv(W, CC_T), ty = cdiv(H, CC_T);
    hipLaunchKernelGGL((cc_tile_label_kernel<T>), dim3(tx * ty, m), dim3(256), 0, stream, masks, index, parent, n, H, W, tx, conn8, invert);
    const long seams = (long)(tx - 1) * H + (long)(ty - 1) * W;
    if (seams > 0) hipLaunchKernelGGL(cc_merge_kernel, dim3(cdiv(seams, 256), m), dim3(256), 0, stream, parent, H, W, tx, ty, conn8);
    hipLaunchKernelGGL(cc_accumulate_kernel, dim3(tx * ty, m), dim3(256), 0, stream, (const int*)parent, root_out, area, border, H, W, tx);
    return 0;
}

extern "C" int psalm_mask_components(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, int connectivity, int invert,
                                     int* labels, int* count, int* table, int max_comp, void* workspace, long workspace_bytes, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0 && H >= 0 && W >= 0, "psalm_mask_components: n, m, H, W >= 0");
    PSALM_CHECK_ARG(connectivity == 4 || connectivity == 8, "psalm_mask_components: connectivity is 4 or 8");
    PSALM_CHECK_ARG(invert == 0 || invert == 1, "psalm_mask_components: invert is 0 or 1");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_components: without an index list the outputs have n rows (m == n)");
    PSALM_CHECK_ARG(table == nullptr || (max_comp >= 1 && max_comp <= 65536), "psalm_mask_components: 1 <= max_comp <= 65536");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_components: at most 65535 output rows");
    PSALM_CHECK_ARG((long)H * W <= INT_MAX, "psalm_mask_components: H * W < 2^31 (pixel indices are int32)");
    PSALM_CHECK_ARG(count != nullptr && ((uintptr_t)count & 3) == 0 && ((uintptr_t)table & 3) == 0, "psalm_mask_components: count / table must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if ((table && hipMemsetAsync(table, 0, (size_t)m * max_comp * 6 * 4, s) != hipSuccess) ||
        ((H == 0 || W == 0) && hipMemsetAsync(count, 0, (size_t)m * 4, s) != hipSuccess)) {
        psalm_set_error("psalm_mask_components: hipMemsetAsync failed");
        return -2;
    }
    if (H == 0 || W == 0) return 0;
    PSALM_CHECK_ARG(labels != nullptr && ((uintptr_t)labels & 3) == 0, "psalm_mask_components: labels must be 4-byte aligned");
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_mask_components_workspace(m, H, W) && ((uintptr_t)workspace & 3) == 0,
                    "psalm_mask_components: workspace of psalm_mask_components_workspace(m, H, W) bytes, 4-byte aligned");
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_components: float32 masks must be 4-byte aligned");
    int* ws = (int*)workspace;
    const long HW = (long)H * W, plane = (long)m * HW;
    const int conn8 = connectivity == 8 ? 1 : 0;
    const int rc = dtype_is_u8 ? cc_label((const unsigned char*)masks, index, n, m, H, W, conn8, invert, ws, labels, s, "psalm_mask_components: hipMemsetAsync failed")
                               : cc_label((const float*)masks, index, n, m, H, W, conn8, invert, ws, labels, s, "psalm_mask_components: hipMemsetAsync failed");
    if (rc) return rc;
    int *parent = ws, *area = ws + plane, *border = ws + 2 * plane, *bsum = ws + 3 * plane;
    const int nb = (int)cc_scan_blocks(H, W);
    hipLaunchKernelGGL(cc_count_roots_kernel, dim3(nb, m), dim3(256), 0, s, (const int*)labels, HW, nb, bsum);
    hipLaunchKernelGGL(cc_scan_blocks_kernel, dim3(m), dim3(256), 0, s, bsum, nb, count);
    hipLaunchKernelGGL(cc_assign_kernel, dim3(nb, m), dim3(256), 0, s, (const int*)labels, (const int*)bsum, (const int*)area, (const int*)border, parent, table,
                       H, W, nb, max_comp);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(cdiv((long)H * cdiv(W, 64), 4), m), dim3(256), 0, s, labels, (const int*)parent, table, H, W, max_comp);
    PSALM_LAUNCH_END("psalm_mask_components");
}

extern "C" int psalm_mask_clean(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, int connectivity, int min_island,
                                int max_hole, unsigned char* out, int* areas, int* filled, int* removed, void* workspace, long workspace_bytes,
                                void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0 && H >= 0 && W >= 0, "psalm_mask_clean: n, m, H, W >= 0");
    PSALM_CHECK_ARG(connectivity == 4 || connectivity == 8, "psalm_mask_clean: connectivity is 4 or 8");
    PSALM_CHECK_ARG(min_island >= 0 && max_hole >= 0, "psalm_mask_clean: min_island, max_hole >= 0");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_clean: without an index list the outputs have n rows (m == n)");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_clean: at most 65535 output rows");
    PSALM_CHECK_ARG((long)H * W <= INT_MAX, "psalm_mask_clean: H * W < 2^31 (pixel indices and areas are int32)");
    PSALM_CHECK_ARG(areas && filled && removed && (((uintptr_t)areas | (uintptr_t)filled | (uintptr_t)removed) & 3) == 0,
                    "psalm_mask_clean: areas / filled / removed must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(areas, 0, (size_t)m * 4, s) != hipSuccess || hipMemsetAsync(filled, 0, (size_t)m * 4, s) != hipSuccess ||
        hipMemsetAsync(removed, 0, (size_t)m * 4, s) != hipSuccess) {
        psalm_set_error("psalm_mask_clean: hipMemsetAsync failed");
        return -2;
    }
    if (H == 0 || W == 0) return 0;
    PSALM_CHECK_ARG(out != nullptr, "psalm_mask_clean: out is NULL");
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_clean: float32 masks must be 4-byte aligned");
    const long HW = (long)H * W, plane = (long)m * HW;
    const dim3 ggrid(cdiv(HW, CC_GATHER), m);
    if (dtype_is_u8) hipLaunchKernelGGL((cc_gather_kernel<unsigned char>), ggrid, dim3(256), 0, s, (const unsigned char*)masks, index, n, HW, out, areas);
    else hipLaunchKernelGGL((cc_gather_kernel<float>), ggrid, dim3(256), 0, s, (const float*)masks, index, n, HW, out, areas);
    if (min_island > 0 || max_hole > 0) {
        PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_mask_clean_workspace(m, H, W) && ((uintptr_t)workspace & 3) == 0,
                        "psalm_mask_clean: workspace of psalm_mask_clean_workspace(m, H, W) bytes, 4-byte aligned");
        int* ws = (int*)workspace;
        const int tx = cdiv(W, CC_T), ty = cdiv(H, CC_T);
        for (int step = 0; step < 2; ++step) {                         // 0: holes (the unset pixels under the complementary connectivity), 1: islands
            const int fill = step == 0 ? 1 : 0, thresh = fill ? max_hole : min_island;
            if (thresh == 0) continue;
            const int conn8 = (connectivity == 8) != (fill != 0) ? 1 : 0;
            const int rc = cc_label((const unsigned char*)out, nullptr, m, m, H, W, conn8, fill, ws, nullptr, s, "psalm_mask_clean: hipMemsetAsync failed");
            if (rc) return rc;
            hipLaunchKernelGGL(cc_decide_kernel, dim3(tx * ty, m), dim3(256), 0, s, (const int*)ws, (const int*)(ws + plane), (const int*)(ws + 2 * plane), out,
                               fill ? filled : removed, areas, H, W, tx, fill, thresh);
        }
    }
    PSALM_LAUNCH_END("psalm_mask_clean");
}
