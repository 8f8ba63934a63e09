// Mask outlines on the device and back (psalm_amd/evalout.py mask_outlines / fill_polygons, PSALM.segment_everything(outlines=True), polygon
// prompts of image sessions): the boundary of every plane as closed rings of lattice corners, and the even-odd fill of such rings.
//   psalm_mask_outline_totals  masks (n,H,W) f32 | u8 (+ an index list) -> counts (3,m) i32 = [crack edges | ring corners | 0] per plane: local sums
//   psalm_mask_outlines        the same planes, rows [row0, row0 + rows) -> ring_count, rings (R,4) i32 = [plane row, first vertex, vertices, signed
//                              area], vertices (V,2) i32 = (x, y)
//   psalm_mask_fill_polygons   rings / vertices in that layout -> out (rows,H,W) bytes of 0 / 1, even-odd over pixel centres
// The definitions (include/psalm_hip.h has them in full): pixel (py, px) covers [px, px + 1] x [py, py + 1]; a crack edge is a unit lattice segment
// between a set and an unset pixel, directed with the set pixel on its right (x to the right, y downwards); directions 0: +x, 1: +y, 2: -x, 3: -y, so
// that "left" of d is (d + 3) & 3.  At its end vertex an edge continues with the first existing of left, straight, right (connectivity 8) or right,
// straight, left (4): every edge has one successor and one predecessor, the edges fall into rings.
//
// A vertex has at most two outgoing edges; its 2 x 2 pixels give them (and whether the edge that arrives in the same direction exists, i.e. whether
// the vertex is a corner of the ring that leaves in that direction -- at a saddle both rings turn).  Launches of psalm_mask_outlines, none waits
// for another block, none reads a word that another block writes in the same launch:
//   1 ol_mask_kernel          a byte per vertex (out | in << 4) and the edges per block of OL_SCAN vertices
//   2 ol_scan_kernel          one block per plane: exclusive scan of the block sums
//   3 ol_link_kernel          voff[v] = number of edges in front of vertex v; edge id = voff[v] + rank among v's directions, so that ids ascend
//                             with the vertex-major key v * 4 + dir: ekey[id] = key
//   4 ol_succ_kernel          per edge: the successor's id from the byte and voff of the end vertex; state[0][e] = {succ, e, 0, corner(e)}
//   5 ol_jump_kernel x R      pointer jumping, ONE LAUNCH PER ROUND from one state array into the other: after round k, state[e] describes the window
//                             of 2^k edges from e on: nxt = the edge behind the window, mn = the smallest id in it, d = the corners in front of
//                             mn's first occurrence, w = the corners of the whole window.  2^R >= the plane's edges: mn is the ring's LEADER (the edge
//                             that leaves the ring's row-major lowest vertex), d the corners from e forward to the leader
//   6 ol_leader_count_kernel  leaders and their rings' corner totals (d of the leader's successor + 1) per block of OL_SCAN edges
//   7 ol_scan_kernel, ol_base_kernel   the same scan over both sums numbers the rings in key order -- the order of their first vertices -- and gives
//                             every ring its first vertex offset; the planes' bases are the prefix sums of the per-plane counts
//   8 ol_assign_kernel        a leader writes its ring's table row and leaves [ring, first vertex, corners] in the dead state array at its own id
//   9 ol_emit_kernel          a corner edge writes its start vertex to first + (corners - d) % corners; a vertical edge adds x dy to the ring's area
//                             (integer atomic add, one per wavefront when the wavefront's edges share the ring)
// The host knows the edge totals (the one read-back of psalm_mask_outline_totals' result) before it calls: grids, R and the workspace follow the
// planes' real boundary length, not H W.  Every loop bound is a launch argument.
#include "common.h"
#include "psalm_hip.h"      // the entries below are checked against their declarations

#include <climits>

#define OL_SCAN 1024                // vertices / edges per block of the scans, 4 consecutive ones per thread

struct __attribute__((aligned(16))) OlState {
    int nxt, mn, d, w;
};

template <typename T> __device__ __forceinline__ bool ol_set(T v);
template <> __device__ __forceinline__ bool ol_set<float>(float v) { return v > 0.f; }               // NaN, -0.0, negatives: not set
template <> __device__ __forceinline__ bool ol_set<unsigned char>(unsigned char v) { return v != 0; }

// vertex (x, y), 0 <= x <= W, 0 <= y <= H: bits 0..3 the outgoing edges by direction, bits 4..7 the incoming ones (by their own direction)
template <typename T>
__device__ __forceinline__ unsigned ol_vertex_bits(const T* base, bool valid, int H, int W, int x, int y) {
    if (!valid) return 0;
    const bool a = x > 0 && y > 0 && ol_set<T>(base[(long)(y - 1) * W + x - 1]);                     // a b
    const bool b = x < W && y > 0 && ol_set<T>(base[(long)(y - 1) * W + x]);                         // c d   around the vertex
    const bool c = x > 0 && y < H && ol_set<T>(base[(long)y * W + x - 1]);
    const bool d = x < W && y < H && ol_set<T>(base[(long)y * W + x]);
    return (d && !b ? 1u : 0u) | (c && !d ? 2u : 0u) | (a && !c ? 4u : 0u) | (b && !a ? 8u : 0u) |
           (c && !a ? 16u : 0u) | (a && !b ? 32u : 0u) | (b && !d ? 64u : 0u) | (d && !c ? 128u : 0u);
}
__device__ __forceinline__ int ol_edges(unsigned bits) { return __builtin_popcount(bits & 15u); }
__device__ __forceinline__ int ol_corners(unsigned bits) { return __builtin_popcount(bits & ~(bits >> 4) & 15u); }

// exclusive scan of v over the block's 256 threads (s: 512 ints of LDS); total = the block's sum
__device__ __forceinline__ int ol_block_scan(int v, int* s, int tid, int& total) {
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

// ---------------------------------------------------------------- totals: what the host sizes the call with
// grid (nbv, m): counts[row] += edges, counts[m + row] += corners (zeroed by the entry); one pair of atomics per block
template <typename T>
__global__ void __launch_bounds__(256) ol_totals_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, int H, int W, int m,
                                                        int* __restrict__ counts) {
    __shared__ int s_e, s_c;
    const int tid = threadIdx.x, row = blockIdx.y;
    if (tid == 0) s_e = s_c = 0;
    __syncthreads();
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;
    const T* base = masks + (valid ? (long)plane * H * W : 0);
    const int W1 = W + 1;
    const long NV = (long)(H + 1) * W1, v0 = (long)blockIdx.x * OL_SCAN + 4 * tid;
    int e = 0, c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v0 + k >= NV) break;
        const unsigned bits = ol_vertex_bits<T>(base, valid, H, W, (int)((v0 + k) % W1), (int)((v0 + k) / W1));
        e += ol_edges(bits);
        c += ol_corners(bits);
    }
    if (e) {
        atomicAdd(&s_e, e);
        atomicAdd(&s_c, c);
    }
    __syncthreads();
    if (tid == 0 && s_e) {
        atomicAdd(&counts[row], s_e);
        atomicAdd(&counts[m + row], s_c);
    }
}

// ---------------------------------------------------------------- 1: vertex bytes, edges per block
// grid (nbv, rows)
template <typename T>
__global__ void __launch_bounds__(256) ol_mask_kernel(const T* __restrict__ masks, const int* __restrict__ index, int row0, int n, int H, int W,
                                                      unsigned char* __restrict__ vm, int nbv, int* __restrict__ bsum) {
    __shared__ int s_e;
    const int tid = threadIdx.x, row = blockIdx.y;
    if (tid == 0) s_e = 0;
    __syncthreads();
    const int plane = index ? index[row0 + row] : row0 + row;
    const bool valid = (unsigned)plane < (unsigned)n;
    const T* base = masks + (valid ? (long)plane * H * W : 0);
    const int W1 = W + 1;
    const long NV = (long)(H + 1) * W1, v0 = (long)blockIdx.x * OL_SCAN + 4 * tid;
    int e = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v0 + k >= NV) break;
        const unsigned bits = ol_vertex_bits<T>(base, valid, H, W, (int)((v0 + k) % W1), (int)((v0 + k) / W1));
        vm[(long)row * NV + v0 + k] = (unsigned char)bits;
        e += ol_edges(bits);
    }
    if (e) atomicAdd(&s_e, e);
    __syncthreads();
    if (tid == 0) bsum[(long)row * nbv + blockIdx.x] = s_e;
}

// ---------------------------------------------------------------- 2 / 7: scan of the block sums
// grid (rows), one block per plane: a[row] (and b[row] when given) become their own exclusive scans; total_a[row] (when given) = the sum of a
__global__ void __launch_bounds__(256) ol_scan_kernel(int* __restrict__ a, int* __restrict__ b, int nb, int* __restrict__ total_a) {
    __shared__ int s[512];
    const int tid = threadIdx.x;
    int* pa = a + (long)blockIdx.x * nb;
    int* pb = b ? b + (long)blockIdx.x * nb : nullptr;
    int ca = 0, cb = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {                             // block-uniform trip count
        const bool in = c0 + tid < nb;
        int total;
        const int va = in ? pa[c0 + tid] : 0;
        const int ea = ol_block_scan(va, s, tid, total);
        if (in) pa[c0 + tid] = ca + ea;
        ca += total;
        if (pb) {                                                      // uniform
            const int vb = in ? pb[c0 + tid] : 0;
            const int eb = ol_block_scan(vb, s, tid, total);
            if (in) pb[c0 + tid] = cb + eb;
            cb += total;
        }
    }
    if (tid == 0 && total_a) total_a[blockIdx.x] = ca;
}

// ---------------------------------------------------------------- 3: edge ids
// grid (nbv, rows): voff for every vertex, ekey for every edge (id < cap: the host's bound on a plane's edges)
__global__ void __launch_bounds__(256) ol_link_kernel(const unsigned char* __restrict__ vm, const int* __restrict__ bsum, int nbv, long NV, int cap,
                                                      int* __restrict__ voff, int* __restrict__ ekey) {
    __shared__ int s[512];
    const int tid = threadIdx.x, row = blockIdx.y;
    const long v0 = (long)blockIdx.x * OL_SCAN + 4 * tid;
    unsigned bits[4];
    int e = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bits[k] = v0 + k < NV ? (vm[(long)row * NV + v0 + k] & 15u) : 0u;
        e += __builtin_popcount(bits[k]);
    }
    int total;
    int id = bsum[(long)row * nbv + blockIdx.x] + ol_block_scan(e, s, tid, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v0 + k >= NV) break;
        voff[(long)row * NV + v0 + k] = id;
        for (int dir = 0; dir < 4; ++dir)
            if ((bits[k] >> dir) & 1u) {
                if (id < cap) ekey[(long)row * cap + id] = (int)((v0 + k) * 4 + dir);
                ++id;
            }
    }
}

// the id of the edge that follows the edge `key` (of id `self`): at the end vertex the first existing of left, straight, right (8) / right,
// straight, left (4); `self` if the end vertex has none of them (it always has: the guard keeps a broken table from leaving the plane)
__device__ __forceinline__ int ol_successor(const unsigned char* vm, const int* voff, int key, int self, int W1, long NV, int conn8) {
    const int dir = key & 3;
    const long v = key >> 2;
    const long v2 = v + (dir == 0 ? 1 : dir == 1 ? W1 : dir == 2 ? -1 : -W1);
    if (v2 < 0 || v2 >= NV) return self;
    const unsigned out = vm[v2] & 15u;
    const int first = conn8 ? (dir + 3) & 3 : (dir + 1) & 3, last = conn8 ? (dir + 1) & 3 : (dir + 3) & 3;
    const int d2 = ((out >> first) & 1u) ? first : ((out >> dir) & 1u) ? dir : ((out >> last) & 1u) ? last : -1;
    if (d2 < 0) return self;
    return voff[v2] + __builtin_popcount(out & ((1u << d2) - 1u));
}

// ---------------------------------------------------------------- 4: successors, the windows of one edge
// grid (ceil(cap / 256), rows)
__global__ void __launch_bounds__(256) ol_succ_kernel(const unsigned char* __restrict__ vm, const int* __restrict__ voff, const int* __restrict__ ekey,
                                                      const int* __restrict__ edge_count, int row0, int W1, long NV, int cap, int conn8,
                                                      OlState* __restrict__ st) {
    const int row = blockIdx.y, e = (int)blockIdx.x * 256 + threadIdx.x;
    const int E = min(edge_count[row0 + row], cap);
    if (e >= E) return;
    const int key = ekey[(long)row * cap + e];
    int nx = ol_successor(vm + (long)row * NV, voff + (long)row * NV, key, e, W1, NV, conn8);
    if ((unsigned)nx >= (unsigned)E) nx = e;
    OlState o;
    o.nxt = nx;
    o.mn = e;
    o.d = 0;
    o.w = ((vm[(long)row * NV + (key >> 2)] >> (4 + (key & 3))) & 1u) ? 0 : 1;     // no edge arrives in this direction: the vertex is a corner
    st[(long)row * cap + e] = o;
}

// ---------------------------------------------------------------- 5: one round of pointer jumping
// grid (ceil(cap / 256), rows): dst[e] = src[e] joined with src[src[e].nxt] -- reads src only, writes dst only
__global__ void __launch_bounds__(256) ol_jump_kernel(const OlState* __restrict__ src, OlState* __restrict__ dst, const int* __restrict__ edge_count,
                                                      int row0, int cap) {
    const int row = blockIdx.y, e = (int)blockIdx.x * 256 + threadIdx.x;
    const int E = min(edge_count[row0 + row], cap);
    if (e >= E) return;
    const OlState a = src[(long)row * cap + e];
    const OlState b = src[(long)row * cap + a.nxt];                    // a.nxt < E: ol_succ_kernel's guard, and every nxt is some edge's successor
    OlState o;
    o.nxt = b.nxt;
    const bool keep = a.mn <= b.mn;                                    // the FIRST occurrence of the minimum: a window may wrap round its ring
    o.mn = keep ? a.mn : b.mn;
    o.d = keep ? a.d : a.w + b.d;
    o.w = a.w + b.w;
    dst[(long)row * cap + e] = o;
}

// a leader's ring has d(successor) + 1 corners: the successor's corners up to the leader, and the leader's own first vertex
__device__ __forceinline__ int ol_ring_corners(const OlState* fin, const unsigned char* vm, const int* voff, const int* ekey, int e, int E, int W1, long NV,
                                               int conn8) {
    int nx = ol_successor(vm, voff, ekey[e], e, W1, NV, conn8);
    if ((unsigned)nx >= (unsigned)E) nx = e;
    return fin[nx].d + 1;
}

// ---------------------------------------------------------------- 6: leaders per block
// grid (nbe, rows): lsum[row][b] = leaders, vsum[row][b] = their rings' corners among the edges [b OL_SCAN, (b + 1) OL_SCAN)
__global__ void __launch_bounds__(256) ol_leader_count_kernel(const OlState* __restrict__ fin, const unsigned char* __restrict__ vm,
                                                              const int* __restrict__ voff, const int* __restrict__ ekey,
                                                              const int* __restrict__ edge_count, int row0, int W1, long NV, int cap, int conn8, int nbe,
                                                              int* __restrict__ lsum, int* __restrict__ vsum) {
    __shared__ int s_l, s_v;
    const int tid = threadIdx.x, row = blockIdx.y;
    if (tid == 0) s_l = s_v = 0;
    __syncthreads();
    const int E = min(edge_count[row0 + row], cap);
    const OlState* f = fin + (long)row * cap;
    const int e0 = (int)blockIdx.x * OL_SCAN + 4 * tid;
    int l = 0, v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e0 + k < E && f[e0 + k].mn == e0 + k) {
            ++l;
            v += ol_ring_corners(f, vm + (long)row * NV, voff + (long)row * NV, ekey + (long)row * cap, e0 + k, E, W1, NV, conn8);
        }
    if (l) {
        atomicAdd(&s_l, l);
        atomicAdd(&s_v, v);
    }
    __syncthreads();
    if (tid == 0) {
        lsum[(long)row * nbe + blockIdx.x] = s_l;
        vsum[(long)row * nbe + blockIdx.x] = s_v;
    }
}

// ---------------------------------------------------------------- 7: the planes' bases in the output tables
// one block: base_r[row] = sum of ring_count[q], base_v[row] = sum of vertex_count[q] over the output rows q < row0 + row (the whole call's rows
// in front of this one, earlier chunks included: their ring counts were written by earlier launches)
__global__ void __launch_bounds__(256) ol_base_kernel(const int* __restrict__ ring_count, const int* __restrict__ vertex_count, int row0, int rows,
                                                      int* __restrict__ base_r, int* __restrict__ base_v) {
    __shared__ int s[512];
    const int tid = threadIdx.x, end = row0 + rows;
    int cr = 0, cv = 0;
    for (int c0 = 0; c0 < end; c0 += 256) {                            // block-uniform trip count
        const int q = c0 + tid;
        int total;
        const int er = ol_block_scan(q < end ? ring_count[q] : 0, s, tid, total);
        if (q >= row0 && q < end) base_r[q - row0] = cr + er;
        cr += total;
        const int ev = ol_block_scan(q < end ? vertex_count[q] : 0, s, tid, total);
        if (q >= row0 && q < end) base_v[q - row0] = cv + ev;
        cv += total;
    }
}

// ---------------------------------------------------------------- 8: ring table rows
// grid (nbe, rows): a leader's number = the leaders in front of it; info[leader] = {ring row in the table, first vertex, corners, 0}
__global__ void __launch_bounds__(256) ol_assign_kernel(const OlState* __restrict__ fin, OlState* __restrict__ info, const unsigned char* __restrict__ vm,
                                                        const int* __restrict__ voff, const int* __restrict__ ekey, const int* __restrict__ edge_count,
                                                        int row0, int W1, long NV, int cap, int conn8, int nbe, const int* __restrict__ lsum,
                                                        const int* __restrict__ vsum, const int* __restrict__ base_r, const int* __restrict__ base_v,
                                                        int* __restrict__ rings, int ring_cap) {
    __shared__ int s[512];
    const int tid = threadIdx.x, row = blockIdx.y;
    const int E = min(edge_count[row0 + row], cap);
    const OlState* f = fin + (long)row * cap;
    const int e0 = (int)blockIdx.x * OL_SCAN + 4 * tid;
    int corners[4], l = 0, v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        corners[k] = 0;
        if (e0 + k < E && f[e0 + k].mn == e0 + k) {
            corners[k] = ol_ring_corners(f, vm + (long)row * NV, voff + (long)row * NV, ekey + (long)row * cap, e0 + k, E, W1, NV, conn8);
            ++l;
            v += corners[k];
        }
    }
    int total;
    int rn = base_r[row] + lsum[(long)row * nbe + blockIdx.x] + ol_block_scan(l, s, tid, total);
    int vo = base_v[row] + vsum[(long)row * nbe + blockIdx.x] + ol_block_scan(v, s, tid, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!corners[k]) continue;                                     // (a ring has at least 4 corners)
        OlState o;
        o.nxt = rn;
        o.mn = vo;
        o.d = corners[k];
        o.w = 0;
        info[(long)row * cap + e0 + k] = o;
        if (rn < ring_cap) {
            int* t = rings + (long)rn * 4;
            t[0] = row0 + row;
            t[1] = vo;
            t[2] = corners[k];
            t[3] = 0;
        }
        ++rn;
        vo += corners[k];
    }
}

// ---------------------------------------------------------------- 9: corners to their places, areas
// grid (ceil(cap / 256), rows); no thread leaves before the wavefront's shuffles
__global__ void __launch_bounds__(256) ol_emit_kernel(const OlState* __restrict__ fin, const OlState* __restrict__ info, const unsigned char* __restrict__ vm,
                                                      const int* __restrict__ ekey, const int* __restrict__ edge_count, int row0, int W1, long NV, int cap,
                                                      int* __restrict__ rings, int ring_cap, int* __restrict__ vertices, int vertex_cap) {
    const int row = blockIdx.y, e = (int)blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int E = min(edge_count[row0 + row], cap);
    int ring = -1, contrib = 0;
    if (e < E) {
        const OlState st = fin[(long)row * cap + e];
        const OlState in = info[(long)row * cap + st.mn];              // {ring, first vertex, corners, 0} of the ring's leader
        const int key = ekey[(long)row * cap + e], dir = key & 3, x = (key >> 2) % W1, y = (key >> 2) / W1;
        const bool corner = !((vm[(long)row * NV + (key >> 2)] >> (4 + dir)) & 1u);
        if (corner && in.d > 0) {
            const long at = (long)in.mn + (in.d - st.d) % in.d;        // 0 <= st.d < corners; the leader itself has st.d == 0
            if (st.d >= 0 && st.d <= in.d && at >= 0 && at < vertex_cap) {
                vertices[2 * at] = x;
                vertices[2 * at + 1] = y;
            }
        }
        if ((dir & 1) && in.nxt >= 0 && in.nxt < ring_cap) {           // a vertical edge: x dy
            ring = in.nxt;
            contrib = dir == 1 ? x : -x;
        }
    }
    const unsigned long long act = __ballot(ring >= 0 ? 1 : 0);
    if (!act) return;                                                  // wave-uniform
    const int first = __builtin_ctzll(act);
    const int id = __shfl(ring, first);
    if (__ballot(ring == id ? 1 : 0) == act) {                         // the wavefront's vertical edges share one ring: one atomic
        int sum = ring >= 0 ? contrib : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == first && sum) atomicAdd(&rings[(long)id * 4 + 3], sum);
    } else if (ring >= 0 && contrib) {
        atomicAdd(&rings[(long)ring * 4 + 3], contrib);
    }
}

// ---------------------------------------------------------------- the fill: toggles, then parity from the right
// grid (ceil(R / 4)), a wavefront per ring, a lane per edge (lanes stride over long rings): one toggle per crossed pixel-centre row, at the first
// column whose centre is not left of the crossing -- the pixels in front of that column count the edge.  cnt (rows, H, W + 1) i32, zeroed.
__global__ void __launch_bounds__(256) pf_toggle_kernel(const int* __restrict__ rings, int R, const int* __restrict__ vertices, int V, int row0, int rows,
                                                        int H, int W, int* __restrict__ cnt) {
    const int ring = (int)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ring >= R) return;
    const int p = rings[4 * (long)ring] - row0, off = rings[4 * (long)ring + 1], nv = rings[4 * (long)ring + 2];
    if ((unsigned)p >= (unsigned)rows || nv < 1 || off < 0 || (long)off + nv > V) return;
    for (int i = lane; i < nv; i += 64) {
        const int j = i + 1 == nv ? 0 : i + 1;
        long x0 = vertices[2 * ((long)off + i)], y0 = vertices[2 * ((long)off + i) + 1];
        long x1 = vertices[2 * ((long)off + j)], y1 = vertices[2 * ((long)off + j) + 1];
        if (y0 == y1) continue;
        if (y0 > y1) {
            long t = x0; x0 = x1; x1 = t;
            t = y0; y0 = y1; y1 = t;
        }
        const long dy = y1 - y0, dx = x1 - x0;
        const long lo = y0 > 0 ? y0 : 0, hi = y1 < H ? y1 : H;         // 2 y0 <= 2 py + 1 < 2 y1  <=>  y0 <= py < y1
        for (long py = lo; py < hi; ++py) {
            const long a = 2 * x0 * dy + (2 * py + 1 - 2 * y0) * dx - dy, b = 2 * dy;      // pixel px counts the edge iff (2 px + 1) dy < a + dy
            long c = a >= 0 ? (a + b - 1) / b : -((-a) / b);           // ceil(a / b): the first column that does not
            if (c <= 0) continue;
            if (c > W) c = W;
            atomicAdd(&cnt[((long)p * H + py) * (W + 1) + c], 1);
        }
    }
}
// grid (H, rows), a block per pixel row: out[px] = parity of the toggles at the columns > px.  A thread owns ceil((W + 1) / 256) columns.
__global__ void __launch_bounds__(256) pf_parity_kernel(const int* __restrict__ cnt, int H, int W, unsigned char* __restrict__ out) {
    __shared__ int s[512];
    const int tid = threadIdx.x, W1 = W + 1, per = (W1 + 255) / 256;
    const int* c = cnt + ((long)blockIdx.y * H + blockIdx.x) * W1;
    unsigned char* o = out + ((long)blockIdx.y * H + blockIdx.x) * W;
    const int lo = tid * per < W1 ? tid * per : W1, hi = lo + per < W1 ? lo + per : W1;
    int sum = 0;
    for (int x = lo; x < hi; ++x) sum += c[x];
    int total;
    const int ex = ol_block_scan(sum, s, tid, total);
    int run = total - ex - sum;                                        // the toggles right of this thread's columns
    for (int x = hi - 1; x >= lo; --x) {
        if (x < W) o[x] = (unsigned char)(run & 1);
        run += c[x];
    }
}

// ---------------------------------------------------------------- entries
static bool ol_dims_ok(int m, int H, int W) { return m >= 0 && m <= 65535 && H >= 0 && W >= 0 && (long)(H + 1) * (W + 1) * 4 <= INT_MAX; }
static long ol_align(long bytes) { return (bytes + 15) & ~15L; }

extern "C" long psalm_mask_outlines_workspace(int m, int H, int W, int edge_cap) {
    if (!ol_dims_ok(m, H, W)) return -1;
    const long NV = (long)(H + 1) * (W + 1);
    if (edge_cap < 0 || edge_cap > 2 * NV) return -1;
    if (edge_cap == 0) return 0;
    const long nbv = (NV + OL_SCAN - 1) / OL_SCAN, nbe = ((long)edge_cap + OL_SCAN - 1) / OL_SCAN;
    return 2 * (long)m * edge_cap * 16                                  // the two state arrays
           + ol_align((long)m * (NV + nbv + edge_cap + 2 * nbe + 2) * 4)    // voff, vertex block sums, ekey, leader block sums (2), the bases (2)
           + ol_align((long)m * NV);                                    // the vertex bytes
}
extern "C" long psalm_mask_fill_polygons_workspace(int m, int H, int W) {
    if (!ol_dims_ok(m, H, W)) return -1;
    return (long)m * H * (W + 1) * 4;
}

extern "C" int psalm_mask_outline_totals(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, int* counts, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0 && H >= 0 && W >= 0, "psalm_mask_outline_totals: n, m, H, W >= 0");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_outline_totals: without an index list the outputs have n rows (m == n)");
    if (m == 0) return 0;
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_outline_totals: at most 65535 output rows");
    PSALM_CHECK_ARG((long)(H + 1) * (W + 1) * 4 <= INT_MAX, "psalm_mask_outline_totals: (H + 1) * (W + 1) * 4 < 2^31 (edge keys are int32)");
    PSALM_CHECK_ARG(counts != nullptr && ((uintptr_t)counts & 3) == 0, "psalm_mask_outline_totals: counts (3, m) must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)m * 3 * 4, s) != hipSuccess) {
        psalm_set_error("psalm_mask_outline_totals: hipMemsetAsync failed");
        return -2;
    }
    if (H == 0 || W == 0) return 0;
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_outline_totals: float32 masks must be 4-byte aligned");
    const dim3 grid(cdiv((long)(H + 1) * (W + 1), OL_SCAN), m);
    if (dtype_is_u8) hipLaunchKernelGGL((ol_totals_kernel<unsigned char>), grid, dim3(256), 0, s, (const unsigned char*)masks, index, n, H, W, m, counts);
    else hipLaunchKernelGGL((ol_totals_kernel<float>), grid, dim3(256), 0, s, (const float*)masks, index, n, H, W, m, counts);
    PSALM_LAUNCH_END("psalm_mask_outline_totals");
}

extern "C" int psalm_mask_outlines(const void* masks, int dtype_is_u8, int n, int H, int W, const int* index, int m, int row0, int rows, int connectivity,
                                   int edge_cap, int* counts, int* rings, int ring_cap, int* vertices, int vertex_cap, void* workspace,
                                   long workspace_bytes, void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0 && H >= 0 && W >= 0, "psalm_mask_outlines: n, m, H, W >= 0");
    PSALM_CHECK_ARG(connectivity == 4 || connectivity == 8, "psalm_mask_outlines: connectivity is 4 or 8");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_outlines: without an index list the outputs have n rows (m == n)");
    PSALM_CHECK_ARG(row0 >= 0 && rows >= 0 && (long)row0 + rows <= m, "psalm_mask_outlines: rows [row0, row0 + rows) within the m output rows");
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_outlines: at most 65535 output rows");
    PSALM_CHECK_ARG((long)(H + 1) * (W + 1) * 4 <= INT_MAX, "psalm_mask_outlines: (H + 1) * (W + 1) * 4 < 2^31 (edge keys are int32)");
    const long NV = (long)(H + 1) * (W + 1);
    PSALM_CHECK_ARG(edge_cap >= 0 && edge_cap <= 2 * NV, "psalm_mask_outlines: 0 <= edge_cap <= 2 (H + 1) (W + 1)");
    PSALM_CHECK_ARG(ring_cap >= 0 && vertex_cap >= 0, "psalm_mask_outlines: ring_cap, vertex_cap >= 0");
    if (rows == 0 || edge_cap == 0 || H == 0 || W == 0) return 0;      // no edges: the ring counts are the zeros psalm_mask_outline_totals left
    PSALM_CHECK_ARG(counts != nullptr && ((uintptr_t)counts & 3) == 0, "psalm_mask_outlines: counts (3, m) must be 4-byte aligned");
    PSALM_CHECK_ARG((rings != nullptr || ring_cap == 0) && (vertices != nullptr || vertex_cap == 0) && (((uintptr_t)rings | (uintptr_t)vertices) & 3) == 0,
                    "psalm_mask_outlines: rings (ring_cap, 4) / vertices (vertex_cap, 2) must be 4-byte aligned");
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_mask_outlines_workspace(rows, H, W, edge_cap) && ((uintptr_t)workspace & 15) == 0,
                    "psalm_mask_outlines: workspace of psalm_mask_outlines_workspace(rows, H, W, edge_cap) bytes, 16-byte aligned");
    PSALM_CHECK_ARG(masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0), "psalm_mask_outlines: float32 masks must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int cap = edge_cap, W1 = W + 1, conn8 = connectivity == 8 ? 1 : 0;
    const int nbv = cdiv(NV, OL_SCAN), nbe = cdiv(cap, OL_SCAN), gbe = cdiv(cap, 256);
    OlState* st[2] = {(OlState*)workspace, (OlState*)workspace + (long)rows * cap};
    int* voff = (int*)(st[1] + (long)rows * cap);
    int *bsum = voff + (long)rows * NV, *ekey = bsum + (long)rows * nbv, *lsum = ekey + (long)rows * cap, *vsum = lsum + (long)rows * nbe;
    int *base_r = vsum + (long)rows * nbe, *base_v = base_r + rows;
    unsigned char* vm = (unsigned char*)voff + ol_align((long)rows * (NV + nbv + cap + 2 * nbe + 2) * 4);
    const int *edge_count = counts, *vertex_count = counts + m;
    int* ring_count = counts + 2 * (long)m;

    if (dtype_is_u8)
        hipLaunchKernelGGL((ol_mask_kernel<unsigned char>), dim3(nbv, rows), dim3(256), 0, s, (const unsigned char*)masks, index, row0, n, H, W, vm, nbv, bsum);
    else hipLaunchKernelGGL((ol_mask_kernel<float>), dim3(nbv, rows), dim3(256), 0, s, (const float*)masks, index, row0, n, H, W, vm, nbv, bsum);
    hipLaunchKernelGGL(ol_scan_kernel, dim3(rows), dim3(256), 0, s, bsum, (int*)nullptr, nbv, (int*)nullptr);
    hipLaunchKernelGGL(ol_link_kernel, dim3(nbv, rows), dim3(256), 0, s, (const unsigned char*)vm, (const int*)bsum, nbv, NV, cap, voff, ekey);
    hipLaunchKernelGGL(ol_succ_kernel, dim3(gbe, rows), dim3(256), 0, s, (const unsigned char*)vm, (const int*)voff, (const int*)ekey, edge_count, row0, W1, NV,
                       cap, conn8, st[0]);
    int R = 0;
    while ((1L << R) < cap) ++R;                                       // 2^R >= the longest possible ring
    for (int r = 0; r < R; ++r)
        hipLaunchKernelGGL(ol_jump_kernel, dim3(gbe, rows), dim3(256), 0, s, (const OlState*)st[r & 1], st[(r & 1) ^ 1], edge_count, row0, cap);
    const OlState* fin = st[R & 1];
    OlState* info = st[(R & 1) ^ 1];
    hipLaunchKernelGGL(ol_leader_count_kernel, dim3(nbe, rows), dim3(256), 0, s, fin, (const unsigned char*)vm, (const int*)voff, (const int*)ekey, edge_count,
                       row0, W1, NV, cap, conn8, nbe, lsum, vsum);
    hipLaunchKernelGGL(ol_scan_kernel, dim3(rows), dim3(256), 0, s, lsum, vsum, nbe, ring_count + row0);
    hipLaunchKernelGGL(ol_base_kernel, dim3(1), dim3(256), 0, s, (const int*)ring_count, vertex_count, row0, rows, base_r, base_v);
    hipLaunchKernelGGL(ol_assign_kernel, dim3(nbe, rows), dim3(256), 0, s, fin, info, (const unsigned char*)vm, (const int*)voff, (const int*)ekey, edge_count,
                       row0, W1, NV, cap, conn8, nbe, (const int*)lsum, (const int*)vsum, (const int*)base_r, (const int*)base_v, rings, ring_cap);
    hipLaunchKernelGGL(ol_emit_kernel, dim3(gbe, rows), dim3(256), 0, s, fin, (const OlState*)info, (const unsigned char*)vm, (const int*)ekey, edge_count,
                       row0, W1, NV, cap, rings, ring_cap, vertices, vertex_cap);
    PSALM_LAUNCH_END("psalm_mask_outlines");
}

extern "C" int psalm_mask_fill_polygons(const int* rings, int R, const int* vertices, int V, int row0, int rows, int H, int W, unsigned char* out,
                                        void* workspace, long workspace_bytes, void* stream) {
    PSALM_CHECK_ARG(R >= 0 && V >= 0 && row0 >= 0 && rows >= 0 && H >= 0 && W >= 0, "psalm_mask_fill_polygons: R, V, row0, rows, H, W >= 0");
    if (rows == 0 || H == 0 || W == 0) return 0;
    PSALM_CHECK_ARG(rows <= 65535, "psalm_mask_fill_polygons: at most 65535 planes per call");
    PSALM_CHECK_ARG((long)(H + 1) * (W + 1) * 4 <= INT_MAX, "psalm_mask_fill_polygons: (H + 1) * (W + 1) * 4 < 2^31");
    PSALM_CHECK_ARG(out != nullptr, "psalm_mask_fill_polygons: out is NULL");
    PSALM_CHECK_ARG((rings != nullptr || R == 0) && (vertices != nullptr || V == 0) && (((uintptr_t)rings | (uintptr_t)vertices) & 3) == 0,
                    "psalm_mask_fill_polygons: rings (R, 4) / vertices (V, 2) must be 4-byte aligned");
    PSALM_CHECK_ARG(workspace != nullptr && workspace_bytes >= psalm_mask_fill_polygons_workspace(rows, H, W) && ((uintptr_t)workspace & 3) == 0,
                    "psalm_mask_fill_polygons: workspace of psalm_mask_fill_polygons_workspace(rows, H, W) bytes, 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, (size_t)rows * H * (W + 1) * 4, s) != hipSuccess) {
        psalm_set_error("psalm_mask_fill_polygons: hipMemsetAsync failed");
        return -2;
    }
    if (R > 0) hipLaunchKernelGGL(pf_toggle_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, rings, R, vertices, V, row0, rows, H, W, (int*)workspace);
    hipLaunchKernelGGL(pf_parity_kernel, dim3(H, rows), dim3(256), 0, s, (const int*)workspace, H, W, out);
    PSALM_LAUNCH_END("psalm_mask_fill_polygons");
}
