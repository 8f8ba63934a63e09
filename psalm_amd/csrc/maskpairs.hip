// All-pairs mask overlap on the device (PSALM.segment_everything, psalm_amd/evalout.py mask_pair_counts / mask_nms): "show me all the objects"
// puts a grid of clicks on an image and gets R picked masks full of duplicates; removing them needs R x R mask IoUs.  The masks are packed into
// BIT PLANES once -- 32 x fewer bytes than fp32 planes, 8 x fewer than bytes: 1024 candidates at 1024^2 are 128 MB, the operand set of the pair
// kernel stays in the last-level cache -- and everything behind that works on 64-pixel words:
//   psalm_mask_pack_bits     masks (n,HW) f32 | u8 (+ an index list naming the planes) -> bits (m,nw) u64, areas (m) i32
//   psalm_mask_unpack_bits   bit rows -> (k,HW) bytes of 0 / 1
//   psalm_mask_pair_counts   inter (ma,mb) i32 = popcount(a_i & b_j) over the words: a small integer "GEMM", tiled in LDS, K split over blocks
//   psalm_mask_nms           greedy NMS on (inter, areas, scores) under an exact rational IoU threshold -> kept list, keep flags, owners
//   psalm_mask_paint_bits    label map (HW) i32 from the kept rows: the best-scoring mask wins a contested pixel
// Layout, plane-flat: word w, bit b of a plane is pixel 64 w + b in row-major order, nw = ceil(HW / 64), the unused high bits of the last word
// are ZERO (every consumer relies on it).  All integer work; partial sums meet in integer atomics: exact, independent of the order of arrival.
#include "common.h"

#include <climits>

typedef unsigned long long mp_u64;

#define MP_PACK_WORDS 256           // words of a plane per block of psalm_mask_pack_bits (16384 pixels)
#define MP_TILE 64                  // pair tile: MP_TILE x MP_TILE pairs per block, 4 x 4 per lane
#define MP_KC 32                    // words of both operands staged in LDS per step
#define MP_LD (MP_TILE + 2)         // LDS row pitch in words: the transposing stores land on 16 different bank pairs, rows stay 16-byte aligned
#define MP_KS 64                    // least number of words per K split (two LDS steps)
#define MP_BLOCKS 1024              // K is split until about this many blocks are in flight
#define MP_MAX 1024                 // most candidates of psalm_mask_pair_counts (per side) and psalm_mask_nms

template <typename T> __device__ __forceinline__ bool mp_set(T v);
template <> __device__ __forceinline__ bool mp_set<float>(float v) { return v > 0.f; }               // NaN, -0.0, negatives: not set
template <> __device__ __forceinline__ bool mp_set<unsigned char>(unsigned char v) { return v != 0; }

// the V = 16 / sizeof(T) elements of one aligned 16-byte word -> bit k = element k is set
__device__ __forceinline__ unsigned mp_vec_bits(const float* p) {
    const psalm_f32x4 a = *reinterpret_cast<const psalm_f32x4*>(p);
    return (a.x > 0.f ? 1u : 0u) | (a.y > 0.f ? 2u : 0u) | (a.z > 0.f ? 4u : 0u) | (a.w > 0.f ? 8u : 0u);
}
__device__ __forceinline__ unsigned mp_vec_bits(const unsigned char* p) {
    const psalm_u32x4 a = *reinterpret_cast<const psalm_u32x4*>(p);
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) bits |= ((w[i] >> (8 * k)) & 0xffu) ? 1u << (4 * i + k) : 0u;
    return bits;
}

// ---------------------------------------------------------------- pack
// grid (word groups, m output rows), block = 4 wavefronts.  A wavefront takes 64 V pixels = V output words at a time: lane l reads the V pixels
// 64 V c + V l .. with ONE 16-byte load when the plane's base is 16-byte aligned (a block-uniform test) and the V pixels lie inside the plane, and
// element by element otherwise (a misaligned plane, the last pixels).  Word j of the V is pixels 64 j .. 64 j + 63, i.e. bit (l % V) of the flags
// of lane (64 / V) j + l / V: one shuffle and ONE ballot per 64 pixels; lane j keeps word j and the first V lanes store.  Pixels at or beyond HW
// are never set, so the last word's tail is zero; a plane index outside [0, n) gives zero words.
template <typename T>
__global__ void __launch_bounds__(256) mask_pack_bits_kernel(const T* __restrict__ masks, const int* __restrict__ index, int n, long HW, long nw,
                                                             mp_u64* __restrict__ bits, int* __restrict__ areas) {
    constexpr int V = 16 / (int)sizeof(T);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.y;
    const int plane = index ? index[row] : row;
    const bool valid = (unsigned)plane < (unsigned)n;                  // block-uniform
    const T* base = masks + (valid ? (long)plane * HW : 0);
    const bool aligned = ((uintptr_t)base & 15) == 0;                  // block-uniform
    const long w0 = (long)blockIdx.x * MP_PACK_WORDS;
    const long w_end = min(nw, w0 + MP_PACK_WORDS);
    int cnt = 0;
    for (long wc = w0 + (long)wave * V; wc < w_end; wc += 4 * V) {     // wave-uniform trip count
        const long p = 64 * wc + (long)V * lane;
        unsigned f = 0;
        if (valid) {
            if (aligned && p + V <= HW) f = mp_vec_bits(base + p);
            else {
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (p + k < HW && mp_set<T>(base[p + k])) f |= 1u << k;
            }
        }
        cnt += __builtin_popcount(f);
        mp_u64 mine = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const unsigned g = __shfl(f, (64 / V) * j + lane / V);
            const mp_u64 word = __ballot((g >> (lane % V)) & 1u);
            if (lane == j) mine = word;
        }
        if (lane < V && wc + lane < w_end) bits[(long)row * nw + wc + lane] = mine;
    }
    if (areas) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0 && cnt) atomicAdd(&areas[row], cnt);
    }
}

// ---------------------------------------------------------------- unpack
// one thread per 16 pixels (a quarter word): a 16-byte store where the address allows, bytes otherwise; grid (groups of 4096 pixels, k rows)
__global__ void __launch_bounds__(256) mask_unpack_bits_kernel(const mp_u64* __restrict__ bits, long nw, const int* __restrict__ rows, long HW,
                                                               unsigned char* __restrict__ out) {
    const int i = blockIdx.y;
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p >= HW) return;
    const int r = rows ? rows[i] : i;
    const unsigned b = r < 0 ? 0u : (unsigned)((bits[(long)r * nw + (p >> 6)] >> (p & 63)) & 0xffffu);
    unsigned char* o = out + (long)i * HW + p;
    if (p + 16 <= HW && ((uintptr_t)o & 15) == 0) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned nib = (b >> (4 * q)) & 0xfu;
            w[q] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
        }
        *reinterpret_cast<psalm_u32x4*>(o) = psalm_u32x4{w[0], w[1], w[2], w[3]};
    } else {
        for (int k = 0; k < 16 && p + k < HW; ++k) o[k] = (unsigned char)((b >> k) & 1u);
    }
}

// ---------------------------------------------------------------- pair counts
// grid (tiles of b, tiles of a, K splits), block 256.  A block owns MP_TILE x MP_TILE pairs over the words [z ks, (z + 1) ks): per step it stages
// MP_KC words of its 64 rows of a and of b in LDS, TRANSPOSED ([word][row], rows beyond ma / mb and words beyond the split as zeros), so that the
// inner loop reads, per word, 4 consecutive rows of a (the same address for the 16 lanes that share them) and 4 of b (512 consecutive bytes per
// 16 lanes) as 16-byte LDS loads and feeds 16 and + popcount pairs from them.  Lane (ti, tj) = (tid / 16, tid % 16) keeps the 4 x 4 counts of rows
// 4 ti .. of a against 4 tj .. of b in registers and adds the non-zero ones into `inter` (zeroed by the entry) with integer atomics.
struct alignas(16) mp_u64x2 { mp_u64 x, y; };
__global__ void __launch_bounds__(256) mask_pair_counts_kernel(const mp_u64* __restrict__ A, int ma, const mp_u64* __restrict__ B, int mb, long nw,
                                                               long ks, int* __restrict__ inter) {
    __shared__ mp_u64x2 sA[MP_KC * MP_LD / 2], sB[MP_KC * MP_LD / 2];
    mp_u64* a_lds = reinterpret_cast<mp_u64*>(sA);
    mp_u64* b_lds = reinterpret_cast<mp_u64*>(sB);
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.y * MP_TILE, j0 = blockIdx.x * MP_TILE;
    const long k_begin = (long)blockIdx.z * ks, k_end = min(nw, k_begin + ks);
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    for (long k0 = k_begin; k0 < k_end; k0 += MP_KC) {                 // block-uniform trip count
        __syncthreads();                                               // the previous step's reads are done
#pragma unroll
        for (int e = tid; e < MP_TILE * MP_KC; e += 256) {             // 8 words of each operand per thread; 32 consecutive lanes read 256 bytes of a row
            const int r = e / MP_KC, k = e % MP_KC;
            const bool in_k = k0 + k < k_end;
            a_lds[k * MP_LD + r] = (in_k && i0 + r < ma) ? A[(long)(i0 + r) * nw + k0 + k] : 0ull;
            b_lds[k * MP_LD + r] = (in_k && j0 + r < mb) ? B[(long)(j0 + r) * nw + k0 + k] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < MP_KC; ++k) {
            const mp_u64x2 a01 = sA[(k * MP_LD + 4 * ti) / 2], a23 = sA[(k * MP_LD + 4 * ti) / 2 + 1];
            const mp_u64x2 b01 = sB[(k * MP_LD + 4 * tj) / 2], b23 = sB[(k * MP_LD + 4 * tj) / 2 + 1];
            const mp_u64 a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += __builtin_popcountll(a[r] & b[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + 4 * ti + r, j = j0 + 4 * tj + c;
            if (i < ma && j < mb && acc[r][c]) atomicAdd(&inter[(long)i * mb + j], acc[r][c]);
        }
}

// ---------------------------------------------------------------- greedy NMS
// One block.  Ranks by counting (descending score, equal scores: the lower index first), then the walk in rank order: a filtered or already
// suppressed candidate is passed over; a kept one marks, in parallel over all candidates, those still undecided that it suppresses -- the walk
// being in rank order, the kept candidate that marks one is the FIRST kept that suppresses it, and a suppressed candidate never gets to mark
// anything.  One barrier per kept candidate.  state: 0 undecided, 1 kept, 2 suppressed, 3 filtered.
__global__ void __launch_bounds__(256) mask_nms_kernel(const int* __restrict__ inter, const int* __restrict__ areas, const float* __restrict__ scores,
                                                       int m, int thr_num, int thr_den, int min_area, float min_score, int* __restrict__ kept,
                                                       int* __restrict__ keep, int* __restrict__ owner) {
    __shared__ float s_score[MP_MAX];
    __shared__ int s_area[MP_MAX], s_order[MP_MAX], s_state[MP_MAX], s_owner[MP_MAX];
    const int tid = threadIdx.x;
    for (int i = tid; i < m; i += 256) {
        s_score[i] = scores[i];
        s_area[i] = areas[i];
        s_order[i] = i;                                                // (ranks are a permutation unless a score is NaN: every slot holds an index all the same)
    }
    __syncthreads();
    for (int i = tid; i < m; i += 256) {
        const float s = s_score[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += (s_score[j] > s || (s_score[j] == s && j < i)) ? 1 : 0;
        s_order[rank] = i;
        const bool filtered = s_area[i] < min_area || s < min_score;
        s_state[i] = filtered ? 3 : 0;
        s_owner[i] = -1;
    }
    __syncthreads();
    int K = 0;                                                         // block-uniform: every thread walks the same list
    for (int t = 0; t < m; ++t) {
        const int i = s_order[t];
        if (s_state[i] != 0) continue;                                 // block-uniform (written before the last barrier)
        __syncthreads();                                               // every thread has read s_state[i] == 0
        if (tid == 0) {
            s_state[i] = 1;
            s_owner[i] = i;
            kept[1 + K] = i;
        }
        ++K;
        const long long ai = s_area[i];
        for (int c = tid; c < m; c += 256) {
            if (c == i || s_state[c] != 0) continue;
            const long long x = inter[(long)c * m + i];                // inter[candidate][kept], as the rule is written
            const long long uni = (long long)s_area[c] + ai - x;
            if ((long long)thr_den * x > (long long)thr_num * uni) {   // IoU > thr_num / thr_den; false at equality and for a zero union
                s_state[c] = 2;
                s_owner[c] = i;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < m; i += 256) {
        const int st = s_state[i];
        keep[i] = st == 1 ? 1 : st == 2 ? 0 : -1;
        owner[i] = s_owner[i];
        if (i >= K) kept[1 + i] = -1;
    }
    if (tid == 0) kept[0] = K;
}

// ---------------------------------------------------------------- paint
// one lane per pixel, so a wavefront shares its word of every kept row (one address per load); the kept list (read on the device: no host sync
// in front of this call) is staged in LDS.  labels[p] = 1 + the first k whose row has pixel p set, 0 if none; pixels >= HW are not written.
__global__ void __launch_bounds__(256) mask_paint_bits_kernel(const mp_u64* __restrict__ bits, long nw, const int* __restrict__ kept, int m, long HW,
                                                              int* __restrict__ labels) {
    __shared__ int s_kept[MP_MAX];
    const int tid = threadIdx.x;
    const int K = max(0, min(kept[0], m));
    for (int k = tid; k < K; k += 256) s_kept[k] = kept[1 + k];
    __syncthreads();
    const long p = (long)blockIdx.x * 256 + tid;
    if (p >= HW) return;
    const long w = p >> 6;
    const int b = (int)(p & 63);
    int label = 0;
    for (int k = 0; k < K; ++k) {
        const int r = s_kept[k];
        if ((unsigned)r < (unsigned)m && ((bits[(long)r * nw + w] >> b) & 1ull)) {       // (m bit rows)
            label = k + 1;
            break;
        }
    }
    labels[p] = label;
}

// ---------------------------------------------------------------- entries
extern "C" long psalm_mask_bits_words(long HW) {
    return (HW > 0 && HW <= INT_MAX) ? (HW + 63) / 64 : -1;
}
extern "C" int psalm_mask_pack_bits(const void* masks, int dtype_is_u8, int n, long HW, const int* index, int m, unsigned long long* bits, int* areas,
                                    void* stream) {
    PSALM_CHECK_ARG(n >= 0 && m >= 0, "psalm_mask_pack_bits: n, m >= 0");
    PSALM_CHECK_ARG(index != nullptr || m == n, "psalm_mask_pack_bits: without an index list the output has n rows (m == n)");
    if (m == 0) return 0;
    const long nw = psalm_mask_bits_words(HW);
    PSALM_CHECK_ARG(nw > 0, "psalm_mask_pack_bits: 0 < HW < 2^31 (the areas are int32)");
    PSALM_CHECK_ARG(m <= 65535, "psalm_mask_pack_bits: at most 65535 output rows");
    PSALM_CHECK_ARG(bits != nullptr && ((uintptr_t)bits & 7) == 0 && ((uintptr_t)areas & 3) == 0,
                    "psalm_mask_pack_bits: bits must be 8-byte aligned, areas 4-byte aligned");
    PSALM_CHECK_ARG(n == 0 || (masks != nullptr && (dtype_is_u8 || ((uintptr_t)masks & 3) == 0)), "psalm_mask_pack_bits: float32 masks must be 4-byte aligned");
    if (areas && hipMemsetAsync(areas, 0, (size_t)m * 4, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_mask_pack_bits: hipMemsetAsync failed");
        return -2;
    }
    const dim3 grid(cdiv(nw, MP_PACK_WORDS), m);
    if (dtype_is_u8) hipLaunchKernelGGL((mask_pack_bits_kernel<unsigned char>), grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)masks, index, n, HW, nw, bits, areas);
    else hipLaunchKernelGGL((mask_pack_bits_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)masks, index, n, HW, nw, bits, areas);
    PSALM_LAUNCH_END("psalm_mask_pack_bits");
}
extern "C" int psalm_mask_unpack_bits(const unsigned long long* bits, long nw, const int* rows, int k, long HW, unsigned char* out, void* stream) {
    PSALM_CHECK_ARG(k >= 0, "psalm_mask_unpack_bits: k >= 0");
    if (k == 0) return 0;
    PSALM_CHECK_ARG(psalm_mask_bits_words(HW) == nw, "psalm_mask_unpack_bits: 0 < HW < 2^31 and nw == psalm_mask_bits_words(HW)");
    PSALM_CHECK_ARG(k <= 65535, "psalm_mask_unpack_bits: at most 65535 output rows");
    PSALM_CHECK_ARG(bits != nullptr && ((uintptr_t)bits & 7) == 0 && out != nullptr, "psalm_mask_unpack_bits: bits must be 8-byte aligned");
    hipLaunchKernelGGL(mask_unpack_bits_kernel, dim3(cdiv(HW, 256 * 16), k), dim3(256), 0, (hipStream_t)stream, (const mp_u64*)bits, nw, rows, HW, out);
    PSALM_LAUNCH_END("psalm_mask_unpack_bits");
}
extern "C" int psalm_mask_pair_counts(const unsigned long long* bits_a, int ma, const unsigned long long* bits_b, int mb, long nw, int* inter,
                                      void* stream) {
    PSALM_CHECK_ARG(ma >= 1 && ma <= MP_MAX && mb >= 1 && mb <= MP_MAX, "psalm_mask_pair_counts: 1 <= ma, mb <= 1024");
    PSALM_CHECK_ARG(nw >= 1 && nw <= (1l << 25), "psalm_mask_pair_counts: 1 <= nw <= 2^25 (the counts are int32)");
    PSALM_CHECK_ARG(bits_a != nullptr && bits_b != nullptr && (((uintptr_t)bits_a | (uintptr_t)bits_b) & 7) == 0 && inter != nullptr &&
                    ((uintptr_t)inter & 3) == 0, "psalm_mask_pair_counts: bits must be 8-byte aligned, inter 4-byte aligned");
    if (hipMemsetAsync(inter, 0, (size_t)ma * mb * 4, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_mask_pair_counts: hipMemsetAsync failed");
        return -2;
    }
    // K split: whole LDS steps, at least MP_KS words, until tiles x splits reaches about MP_BLOCKS (4 blocks per compute unit)
    const int tiles = cdiv(ma, MP_TILE) * cdiv(mb, MP_TILE);
    const long want = tiles >= MP_BLOCKS ? 1 : MP_BLOCKS / tiles;
    long ks = (nw + want - 1) / want;
    ks = (ks + MP_KC - 1) / MP_KC * MP_KC;
    if (ks < MP_KS) ks = MP_KS;
    const dim3 grid(cdiv(mb, MP_TILE), cdiv(ma, MP_TILE), cdiv(nw, ks));
    hipLaunchKernelGGL(mask_pair_counts_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const mp_u64*)bits_a, ma, (const mp_u64*)bits_b, mb, nw, ks, inter);
    PSALM_LAUNCH_END("psalm_mask_pair_counts");
}
extern "C" int psalm_mask_nms(const int* inter, const int* areas, const float* scores, int m, int thr_num, int thr_den, int min_area, float min_score,
                              int* kept, int* keep, int* owner, void* stream) {
    PSALM_CHECK_ARG(m >= 1 && m <= MP_MAX, "psalm_mask_nms: 1 <= m <= 1024");
    PSALM_CHECK_ARG(thr_num > 0 && thr_den > 0 && thr_den <= 4096 && thr_num <= thr_den, "psalm_mask_nms: 0 < thr_num <= thr_den <= 4096");
    PSALM_CHECK_ARG(inter && areas && scores && kept && keep && owner, "psalm_mask_nms: null argument");
    hipLaunchKernelGGL(mask_nms_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, inter, areas, scores, m, thr_num, thr_den, min_area, min_score, kept,
                       keep, owner);
    PSALM_LAUNCH_END("psalm_mask_nms");
}
extern "C" int psalm_mask_paint_bits(const unsigned long long* bits, long nw, const int* kept, int m, long HW, int* labels, void* stream) {
    PSALM_CHECK_ARG(m >= 0 && m <= MP_MAX, "psalm_mask_paint_bits: 0 <= m <= 1024");
    PSALM_CHECK_ARG(psalm_mask_bits_words(HW) == nw, "psalm_mask_paint_bits: 0 < HW < 2^31 and nw == psalm_mask_bits_words(HW)");
    PSALM_CHECK_ARG(bits != nullptr && ((uintptr_t)bits & 7) == 0 && kept != nullptr && labels != nullptr, "psalm_mask_paint_bits: bits must be 8-byte aligned");
    hipLaunchKernelGGL(mask_paint_bits_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, (hipStream_t)stream, (const mp_u64*)bits, nw, kept, m, HW, labels);
    PSALM_LAUNCH_END("psalm_mask_paint_bits");
}
