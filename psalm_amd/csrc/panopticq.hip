// Panoptic quality on the device (psalm_amd/evalout.py label_pair_counts / PanopticQuality): what panopticapi's pq_compute_single_core does on
// the host after the PNG round trip of my_coco_panoptic_evaluator (psalm/eval/segmentation_evaluation/panoptic_evaluation.py:179-221) --
// `np.unique(gt * 256^3 + pred, return_counts=True)` per image, then a match over a table of a few hundred entries -- from id maps that are on
// the device already:
//   psalm_label_pair_counts   two id maps (int32, or the PNG's rgb bytes) + the two sorted id tables -> counts (G+2, P+2) i32, the joint
//                             histogram over (gt slot, pred slot); slot 0 = VOID, 1 + k = table entry k, last = any other value
//   psalm_pq_accumulate       that table + the segments' categories and crowd flags -> tp / fp / fn per category, the matched IoU sums
//                             (float64, added in panopticapi's own order) and a few bookkeeping totals, accumulated over images
// All integer work but the IoU quotients; those are summed by one thread in a fixed order: results are bit-exact against the host formulas
// (tests/test_46_label_pairs_kernels.py).
#include "common.h"

#include <climits>

#define LP_MAX_IDS 1023
#define LP_BLOCK_PIXELS 4096            // pixels of one block's contiguous share, at least (16 per thread)
#define LP_MAX_BLOCKS 1024
#define LP_DENSE_BYTES (144 * 1024)     // LDS budget of the dense table, id tables included (the confusion kernel's budget)
#define LP_HASH_SLOTS 2048              // open-addressed (key, count) table of the sparse form: 16 KB
#define LP_HASH_PROBES 32               // slots looked at before the table counts as full for a key

// slot of pixel value v under the ascending table T of n positive ids: 0 = VOID, 1 + k for T[k], n + 1 for anything else (negatives included)
__device__ __forceinline__ int lp_slot(int v, const int* T, int n) {
    if (v == 0) return 0;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (T[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && T[lo] == v) ? 1 + lo : n + 1;
}
template <bool RGB> __device__ __forceinline__ int lp_load(const void* map, long i) {
    if (RGB) {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(map) + 3 * i;
        return (int)p[0] | ((int)p[1] << 8) | ((int)p[2] << 16);       // panopticapi rgb2id
    }
    return reinterpret_cast<const int*>(map)[i];
}

// Block b counts the pixels [b * chunk, (b + 1) * chunk) (chunk: a multiple of 256), a wavefront 64 consecutive ones at a time.  The lanes
// that hold the same (gt, pred) values as the first unserved lane form a ballot word; its popcount is that pair's count in the segment, and
// the leader alone finds the two slots (binary search of the tables in LDS) and adds the count to the block's table: a segment inside one
// gt / pred region costs one round and one LDS add.  The block's table is
//   DENSE: (G+2) x (P+2) words, flushed with one global add per touched entry;
//   else an open-addressed table of LP_HASH_SLOTS (key + 1, count) pairs -- a block's share touches few pairs of a large table -- claimed
//   with a compare-and-swap; a key that finds neither itself nor a free slot within LP_HASH_PROBES steps adds to global memory directly.
// Integer adds only: the result does not depend on the order of arrival.
// LDS (dynamic): [gt ids (G)] [pred ids (P)] [table].
template <bool GRGB, bool PRGB, bool DENSE>
__global__ void __launch_bounds__(256) label_pair_counts_kernel(const void* __restrict__ gt, const int* __restrict__ gt_ids, int G,
                                                                const void* __restrict__ pred, const int* __restrict__ pred_ids, int P, long n,
                                                                long chunk, unsigned* __restrict__ counts) {
    HIP_DYNAMIC_SHARED(unsigned, lds)
    int* tg = reinterpret_cast<int*>(lds);
    int* tp = tg + G;
    unsigned* tab = lds + G + P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int cols = P + 2, bins = (G + 2) * cols;
    const int words = DENSE ? bins : 2 * LP_HASH_SLOTS;
    for (int i = tid; i < G; i += 256) tg[i] = gt_ids[i];
    for (int i = tid; i < P; i += 256) tp[i] = pred_ids[i];
    for (int i = tid; i < words; i += 256) tab[i] = 0u;
    __syncthreads();
    const long begin = (long)blockIdx.x * chunk;
    const long end = begin + chunk < n ? begin + chunk : n;
    for (long i0 = begin + (tid & ~63); i0 < end; i0 += 256) {          // wave-uniform trip count
        const long i = i0 + lane;
        const bool valid = i < end;
        const int g = valid ? lp_load<GRGB>(gt, i) : 0, p = valid ? lp_load<PRGB>(pred, i) : 0;
        unsigned long long rem = __ballot(valid ? 1 : 0);
        while (rem) {                                                   // wave-uniform
            const int leader = __builtin_ctzll(rem);
            const int kg = __shfl(g, leader), kp = __shfl(p, leader);
            const unsigned long long same = __ballot((valid && g == kg && p == kp) ? 1 : 0);
            if (lane == leader) {
                const unsigned c = (unsigned)__builtin_popcountll(same);
                const unsigned key = (unsigned)(lp_slot(kg, tg, G) * cols + lp_slot(kp, tp, P));          // < bins <= 1025^2
                if (DENSE) atomicAdd(&tab[key], c);
                else {
                    unsigned h = (key * 2654435761u) >> 16;
                    bool placed = false;
                    for (int t = 0; t < LP_HASH_PROBES && !placed; ++t, ++h) {
                        const unsigned s = h & (LP_HASH_SLOTS - 1);
                        const unsigned old = atomicCAS(&tab[2 * s], 0u, key + 1u);
                        if (old == 0u || old == key + 1u) {
                            atomicAdd(&tab[2 * s + 1], c);
                            placed = true;
                        }
                    }
                    if (!placed) atomicAdd(&counts[key], c);
                }
            }
            rem &= ~same;
        }
    }
    __syncthreads();
    if (DENSE) {
        for (int i = tid; i < bins; i += 256)
            if (tab[i]) atomicAdd(&counts[i], tab[i]);
    } else {
        for (int s = tid; s < LP_HASH_SLOTS; s += 256)
            if (tab[2 * s]) atomicAdd(&counts[tab[2 * s] - 1u], tab[2 * s + 1]);
    }
}

template <bool GRGB, bool PRGB>
static void lp_launch(bool dense, int grid, size_t lds, hipStream_t stream, const void* gt, const int* gt_ids, int G, const void* pred,
                      const int* pred_ids, int P, long n, long chunk, unsigned* counts) {
    if (dense) hipLaunchKernelGGL((label_pair_counts_kernel<GRGB, PRGB, true>), dim3(grid), dim3(256), lds, stream, gt, gt_ids, G, pred, pred_ids, P, n, chunk, counts);
    else hipLaunchKernelGGL((label_pair_counts_kernel<GRGB, PRGB, false>), dim3(grid), dim3(256), lds, stream, gt, gt_ids, G, pred, pred_ids, P, n, chunk, counts);
}
extern "C" int psalm_label_pair_counts(const void* gt, int gt_is_rgb, const int* gt_ids, int G, const void* pred, int pred_is_rgb,
                                       const int* pred_ids, int P, int H, int W, int* counts, void* stream) {
    PSALM_CHECK_ARG(G >= 0 && G <= LP_MAX_IDS && P >= 0 && P <= LP_MAX_IDS, "psalm_label_pair_counts: 0 <= G, P <= 1023 listed ids");
    PSALM_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= INT_MAX, "psalm_label_pair_counts: H, W >= 1, H * W < 2^31 (the counts are int32)");
    PSALM_CHECK_ARG(gt != nullptr && pred != nullptr && counts != nullptr && (G == 0 || gt_ids != nullptr) && (P == 0 || pred_ids != nullptr),
                    "psalm_label_pair_counts: null pointer");
    PSALM_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)gt_ids & 3) == 0 && ((uintptr_t)pred_ids & 3) == 0 &&
                        (gt_is_rgb || ((uintptr_t)gt & 3) == 0) && (pred_is_rgb || ((uintptr_t)pred & 3) == 0),
                    "psalm_label_pair_counts: int32 maps / tables must be 4-byte aligned");
    const long n = (long)H * W;
    const int bins = (G + 2) * (P + 2);
    if (hipMemsetAsync(counts, 0, (size_t)bins * 4, (hipStream_t)stream) != hipSuccess) {
        psalm_set_error("psalm_label_pair_counts: hipMemsetAsync failed");
        return -2;
    }
    const bool dense = (size_t)(G + P + bins) * 4 <= LP_DENSE_BYTES;
    const size_t lds = (size_t)(G + P + (dense ? bins : 2 * LP_HASH_SLOTS)) * 4;
    const long want = (n + LP_BLOCK_PIXELS - 1) / LP_BLOCK_PIXELS;
    const int grid = (int)(want < LP_MAX_BLOCKS ? want : LP_MAX_BLOCKS);
    const long chunk = ((n + grid - 1) / grid + 255) / 256 * 256;      // grid * chunk >= n
    hipStream_t s = (hipStream_t)stream;
    unsigned* c = (unsigned*)counts;
    if (gt_is_rgb) {
        if (pred_is_rgb) lp_launch<true, true>(dense, grid, lds, s, gt, gt_ids, G, pred, pred_ids, P, n, chunk, c);
        else lp_launch<true, false>(dense, grid, lds, s, gt, gt_ids, G, pred, pred_ids, P, n, chunk, c);
    } else {
        if (pred_is_rgb) lp_launch<false, true>(dense, grid, lds, s, gt, gt_ids, G, pred, pred_ids, P, n, chunk, c);
        else lp_launch<false, false>(dense, grid, lds, s, gt, gt_ids, G, pred, pred_ids, P, n, chunk, c);
    }
    PSALM_LAUNCH_END("psalm_label_pair_counts");
}

// ---------------------------------------------------------------- match and accumulate (pq_compute_single_core on the overlap table)
// One block.  Row and column sums (the segments' areas) go to LDS; each thread then searches the rows g = tid + 1, tid + 257, ... for pairs
// that match (same category, gt not crowd, 2 * inter > union in integers == iou > 0.5) and leaves per row the first matching column and the
// number of matches; thread 0 alone walks the rows ascending and adds inter / union to iou[cat] -- the (g, p) order of np.unique's keys, so
// the float64 sums equal a host loop's bit for bit.  (Tables that come from two maps give at most one match per row; a row with more is
// walked again by thread 0, in column order.)  FN / FP / notes are integer adds.
// A category slot outside [0, C) or a crowd slot outside [1, G] makes its segment count nothing rather than write out of bounds.
__device__ __forceinline__ bool pq_match(const int* __restrict__ counts, int cols, const int* ag, const int* ap, int g, int p, long long* inter,
                                         long long* uni) {
    const long long it = counts[(long)g * cols + p];
    if (it == 0) return false;
    const long long u = (long long)ap[p] + ag[g] - it - counts[p];
    *inter = it;
    *uni = u;
    return 2 * it > u;
}
__global__ void __launch_bounds__(256) pq_accumulate_kernel(const int* __restrict__ counts, int G, int P, const int* __restrict__ gt_cat,
                                                            const int* __restrict__ gt_crowd, const int* __restrict__ pred_cat,
                                                            const int* __restrict__ pred_crowd_slot, int C, unsigned long long* __restrict__ stat,
                                                            double* __restrict__ iou, unsigned long long* __restrict__ notes) {
    __shared__ int ag[LP_MAX_IDS + 2], ap[LP_MAX_IDS + 2];             // areas: row sums, column sums (<= H * W < 2^31)
    __shared__ int first[LP_MAX_IDS + 1], nmatch[LP_MAX_IDS + 1];      // per gt slot: first matching pred slot, number of matches
    __shared__ int pmatched[LP_MAX_IDS + 1];
    const int tid = threadIdx.x, rows = G + 2, cols = P + 2;
    for (int g = tid; g < rows; g += 256) {
        int s = 0;
        for (int p = 0; p < cols; ++p) s += counts[(long)g * cols + p];
        ag[g] = s;
    }
    for (int p = tid; p < cols; p += 256) {
        int s = 0;
        for (int g = 0; g < rows; ++g) s += counts[(long)g * cols + p];
        ap[p] = s;
        if (p <= P) pmatched[p] = 0;
    }
    __syncthreads();
    for (int g = 1 + tid; g <= G; g += 256) {
        int f = 0, k = 0;
        const int cat = gt_cat[g - 1];
        if (!gt_crowd[g - 1] && cat >= 0 && cat < C)
            for (int p = 1; p <= P; ++p) {
                long long it, u;
                if (pred_cat[p - 1] == cat && pq_match(counts, cols, ag, ap, g, p, &it, &u)) {
                    if (k++ == 0) f = p;
                    pmatched[p] = 1;                                    // (every writer stores 1)
                }
            }
        first[g] = f;
        nmatch[g] = k;
    }
    __syncthreads();
    if (tid == 0) {
        for (int g = 1; g <= G; ++g) {
            if (nmatch[g] == 0) continue;
            const int cat = gt_cat[g - 1];
            for (int p = first[g]; p <= (nmatch[g] == 1 ? first[g] : P); ++p) {
                long long it, u;
                if (pred_cat[p - 1] != cat || !pq_match(counts, cols, ag, ap, g, p, &it, &u)) continue;
                stat[(long)cat * 3] += 1ull;
                iou[cat] += (double)it / (double)u;
            }
        }
        notes[0] += 1ull;
        notes[1] += (unsigned long long)ag[G + 1];
        notes[2] += (unsigned long long)ap[P + 1];
    }
    for (int g = 1 + tid; g <= G; g += 256) {
        const int cat = gt_cat[g - 1];
        if (nmatch[g] == 0 && !gt_crowd[g - 1] && cat >= 0 && cat < C) atomicAdd(&stat[(long)cat * 3 + 2], 1ull);
    }
    for (int p = 1 + tid; p <= P; p += 256) {
        if (pmatched[p]) continue;
        if (ap[p] == 0) { atomicAdd(&notes[3], 1ull); continue; }
        const int cs = pred_crowd_slot[p - 1], cat = pred_cat[p - 1];
        long long it = counts[p];
        if (cs >= 1 && cs <= G) it += counts[(long)cs * cols + p];
        if (2 * it > (long long)ap[p] || cat < 0 || cat >= C) continue;
        atomicAdd(&stat[(long)cat * 3 + 1], 1ull);
    }
}
extern "C" int psalm_pq_accumulate(const int* counts, int G, int P, const int* gt_cat, const int* gt_crowd, const int* pred_cat,
                                   const int* pred_crowd_slot, int C, long long* stat, double* iou, long long* notes, void* stream) {
    PSALM_CHECK_ARG(G >= 0 && G <= LP_MAX_IDS && P >= 0 && P <= LP_MAX_IDS, "psalm_pq_accumulate: 0 <= G, P <= 1023 listed ids");
    PSALM_CHECK_ARG(C >= 1 && C <= 4096, "psalm_pq_accumulate: 1 <= C <= 4096 categories");
    PSALM_CHECK_ARG(counts != nullptr && stat != nullptr && iou != nullptr && notes != nullptr &&
                        (G == 0 || (gt_cat != nullptr && gt_crowd != nullptr)) && (P == 0 || (pred_cat != nullptr && pred_crowd_slot != nullptr)),
                    "psalm_pq_accumulate: null pointer");
    PSALM_CHECK_ARG(((uintptr_t)stat & 7) == 0 && ((uintptr_t)iou & 7) == 0 && ((uintptr_t)notes & 7) == 0 && ((uintptr_t)counts & 3) == 0,
                    "psalm_pq_accumulate: accumulators must be 8-byte aligned, the table 4-byte aligned");
    hipLaunchKernelGGL(pq_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, G, P, gt_cat, gt_crowd, pred_cat, pred_crowd_slot, C,
                       (unsigned long long*)stat, iou, (unsigned long long*)notes);
    PSALM_LAUNCH_END("psalm_pq_accumulate");
}
