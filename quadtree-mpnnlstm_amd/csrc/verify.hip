// Verification of a rollout, computed where the rollout's outputs are: the per-lead-time sums of score()
// (k_score_multi), the per-pixel maps of score_maps() (k_score_maps), the break-up / freeze-up dates of
// event_dates() with the sums of their errors (k_event_scan, k_event_sums), the per-bin probability sums of
// reliability() (k_reliability_multi), the neighbourhood sums of fss() (k_fss_multi) and the ice-edge distances of
// edge_distance() (k_edge_planes, k_edge_search).  All of them read the head's node values through every step's labels (no
// frame is built), none has a gradient, and the six rollout launchers share one host-side setup (score_setup).  The training loss (k_sse, k_loss_multi, k_pool_targets) is in transfer.hip.
#include "qt_common.h"
#include "../../include/qtmpnn_edges.h"

namespace {

// Forecast verification of a rollout: k_loss_multi's reads with more accumulators, kept per (step, clip, tile) and per
// source (the model's node values through the labels, then up to two dense baseline fields), no gradient.
struct ScoreSeg {
    const float* out[16];         // node values of the step (column 0 of rows of out_stride floats)
    const int32_t* labels[16];
    const int32_t* n_dev[16];
    int out_stride[16], N[16];
};
struct ScoreBase {
    const float* f;               // dense field: step z of clip b starts at f + b*clip_stride + z*step_stride
    int64_t clip_stride, step_stride;
};

// Per tile: n, then per source [sum d, sum |d|, sum d^2, hits, over, under]; the correct negatives are n - hits - over - under
// (every counted pixel falls in exactly one of the four classes, and the counts are integers <= 1024: exact in fp32).
template <int S>
__global__ __launch_bounds__(256) void k_score_multi(ScoreSeg sg, const float* __restrict__ y, int64_t y_clip_stride,
                                                     int64_t y_step_stride, ScoreBase b1, ScoreBase b2,
                                                     const uint8_t* __restrict__ pix_mask, float thr, int64_t P, int B,
                                                     float* __restrict__ partial) {
    constexpr int NV = 1 + 6 * S;
    __shared__ float red[4][NV];
    const int b = blockIdx.y, z = blockIdx.z;
    const float* out = sg.out[z];
    const int32_t* labels = sg.labels[z] + (int64_t)b * P;
    const int os = sg.out_stride[z];
    const int rows = qt_rows(sg.n_dev[z], sg.N[z]);
    const float* yz = y + z * y_step_stride + b * y_clip_stride;
    const float* f1 = S > 1 ? b1.f + z * b1.step_stride + b * b1.clip_stride : nullptr;
    const float* f2 = S > 2 ? b2.f + z * b2.step_stride + b * b2.clip_stride : nullptr;
    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t p = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (p >= P) continue;
        const int lab = labels[p];
        if (lab < 0 || lab >= rows || (pix_mask && pix_mask[p])) continue;
        const float t = yz[p];
        const bool ty = t > thr;
        float f[S];
        f[0] = out[(int64_t)lab * os];
        if (S > 1) f[1] = f1[p];
        if (S > 2) f[2] = f2[p];
        acc[0] += 1.0f;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float* a = acc + 1 + 6 * s;
            const float d = f[s] - t;
            const bool tf = f[s] > thr;
            a[0] += d;
            a[1] += fabsf(d);
            a[2] += d * d;
            a[3] += (tf && ty) ? 1.0f : 0.0f;
            a[4] += (tf && !ty) ? 1.0f : 0.0f;
            a[5] += (!tf && ty) ? 1.0f : 0.0f;
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[v] += __shfl_xor(acc[v], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[threadIdx.x >> 6][v] = acc[v];
    }
    __syncthreads();
    if (threadIdx.x < 8 * S) {
        const int s = threadIdx.x >> 3, slot = threadIdx.x & 7;
        auto total = [&](int v) { return (red[0][v] + red[1][v]) + (red[2][v] + red[3][v]); };
        const int v0 = 1 + 6 * s;
        float r;
        if (slot == 0) r = total(0);
        else if (slot < 7) r = total(v0 + slot - 1);
        else r = total(0) - total(v0 + 3) - total(v0 + 4) - total(v0 + 5);
        partial[((((int64_t)z * B + b) * gridDim.x + blockIdx.x) * S + s) * 8 + slot] = r;
    }
}

// Probability verification of a rollout: k_score_multi's reads, sources, counting rule and tile shape, with the forecast value
// binned into K equal bins of [0, 1] and four sums kept per (source, bin): [n, events, sum f, sum (f - o)^2], o = (y > thr).
// Bin of a value: t = f * (float)K (one fp32 rounding), 0 if not t >= 1 (f < 1/K, negative values and NaN), K - 1 if t >= K
// (overshoot, +inf), else (int)t.  Every thread keeps its four pixels' values, squared errors and bins in registers and the
// workgroup walks the bins: for (source, bin) a lane adds the terms of its pixels that fall in the bin and +0 for the others.
// Summation order of the two float sums, fixed by pixel position: per thread its pixels p, p + 256, p + 512, p + 768 of the tile
// in that order (starting from +0), the 64-lane butterfly (xor 32, 16, 8, 4, 2, 1), then (w0 + w1) + (w2 + w3) over the four
// waves.  A wave none of whose pixels is in the bin skips its butterfly: every lane holds +0 there, which is what the butterfly
// would leave.  The two counts are popcounts of wave ballots (integers <= 1024: exact in fp32).  No atomics: the same bits on
// every run, eager or replayed.  A NaN forecast is in bin 0 and makes that bin's two float sums NaN.
template <int S>
__global__ __launch_bounds__(256) void k_reliability_multi(ScoreSeg sg, const float* __restrict__ y, int64_t y_clip_stride,
                                                           int64_t y_step_stride, ScoreBase b1, ScoreBase b2,
                                                           const uint8_t* __restrict__ pix_mask, float thr, int K, int64_t P,
                                                           int B, float* __restrict__ partial) {
    __shared__ float red[4][S * 32 * 4];
    const int b = blockIdx.y, z = blockIdx.z;
    const float* out = sg.out[z];
    const int32_t* labels = sg.labels[z] + (int64_t)b * P;
    const int os = sg.out_stride[z];
    const int rows = qt_rows(sg.n_dev[z], sg.N[z]);
    const float* yz = y + z * y_step_stride + b * y_clip_stride;
    const float* f1 = S > 1 ? b1.f + z * b1.step_stride + b * b1.clip_stride : nullptr;
    const float* f2 = S > 2 ? b2.f + z * b2.step_stride + b * b2.clip_stride : nullptr;
    const float Kf = (float)K;
    float f[S][4], e2[S][4];
    int bin[S][4];                // -1: the pixel is not counted and matches no bin
    bool ev[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = (int64_t)blockIdx.x * 1024 + j * 256 + threadIdx.x;
        bool counted = p < P;
        int lab = -1;
        if (counted) {
            lab = labels[p];
            counted = lab >= 0 && lab < rows && !(pix_mask && pix_mask[p]);
        }
        ev[j] = false;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            f[s][j] = 0.0f;
            e2[s][j] = 0.0f;
            bin[s][j] = -1;
        }
        if (!counted) continue;
        ev[j] = yz[p] > thr;
        const float o = ev[j] ? 1.0f : 0.0f;
        f[0][j] = out[(int64_t)lab * os];
        if (S > 1) f[1][j] = f1[p];
        if (S > 2) f[2][j] = f2[p];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float d = f[s][j] - o;
            e2[s][j] = d * d;
            const float t = f[s][j] * Kf;
            bin[s][j] = !(t >= 1.0f) ? 0 : t >= Kf ? K - 1 : (int)t;
        }
    }
    const int w = threadIdx.x >> 6;
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            int n = 0, e = 0;
            float sf = 0.0f, sq = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = bin[s][j] == k;
                n += __popcll(__ballot(in));
                e += __popcll(__ballot(in && ev[j]));
                sf += in ? f[s][j] : 0.0f;
                sq += in ? e2[s][j] : 0.0f;
            }
            if (n) {              // wave-uniform: n comes from ballots
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    sf += __shfl_xor(sf, d, 64);
                    sq += __shfl_xor(sq, d, 64);
                }
            }
            if ((threadIdx.x & 63) == 0) {
                float* r = red[w] + (s * K + k) * 4;
                r[0] = (float)n;
                r[1] = (float)e;
                r[2] = sf;
                r[3] = sq;
            }
        }
    }
    __syncthreads();
    float* dst = partial + (((int64_t)z * B + b) * gridDim.x + blockIdx.x) * (S * K * 4);
    for (int v = threadIdx.x; v < S * K * 4; v += 256) dst[v] = (red[0][v] + red[1][v]) + (red[2][v] + red[3][v]);
}

// Neighbourhood verification of a rollout (Fractions Skill Score): k_score_multi's reads, sources and counting rule, but a
// pixel is compared through the number of "ice" pixels in the n x n window around it, n = 2h + 1 one of K scales (h <= 16).
// Indicators: I_o(p) = counted(p) && y[p] > thr, I_s(p) = counted(p) && f_s[p] > thr (strict, fp32: a NaN is not ice); a window
// count c_x(p; n) is the sum of I_x over the window, positions outside the frame and uncounted pixels adding 0.  Per
// (source, scale) the tile keeps five integers over its counted centres: [n, events = sum I_o, sum (c_s - c_o)^2, sum c_s^2,
// sum c_o^2].
// One workgroup per (32 x 32 tile of centres, clip, step).  It reads the 64 x 64 patch of the tile with its 16-pixel halo: wave
// w takes patch rows 16w .. 16w + 15, lane l patch column l, and a ballot turns `counted` and every indicator of a patch row
// into one 64-bit word (lanes outside the frame are false): the patch is 64 rows x (S + 2) words of LDS.  Thread t then owns the
// centres (4 (t >> 5) + j, t & 31), j = 0..3 -- one column, four consecutive rows, so their windows share all but six rows --
// and walks the scales: the window's columns are one mask of 2h + 1 bits (patch columns cc + 16 - h .. cc + 16 + h, inside the
// word because h <= 16), a row's part of a count is popcount(word & mask), and the 2h + 4 rows the four windows cover are read
// once each.  The 32 lanes of a half wave read the same word (an LDS broadcast), the halves two different ones.
// Widths: a count is <= 33^2 = 1089, so a centre's term is <= 1089^2 = 33^4 and a tile's sum <= 1024 * 33^4 = 1 214 383 104
// < 2^31: every partial (per thread: four centres; per wave; per tile) is a non-negative int32 below that, (c_s - c_o)^2
// included since both counts are in 0..1089.  The totals over tiles are added in int64 by the caller.
// Reduction: 64-lane butterflies, then (w0 + w1) + (w2 + w3); n and events are popcounts of the centre bits.  Integers, no
// atomics: the same bits on every run, eager or replayed.  Neighbouring tiles (blockIdx.x, x + 1) are dealt to different XCDs, so
// a halo is fetched by up to four L2s; a step's fields are a few tens of KB per clip, and nothing depends on the placement.
struct FssScales {
    int K, h[8];
};

template <int S>
__global__ __launch_bounds__(256) void k_fss_multi(ScoreSeg sg, const float* __restrict__ y, int64_t y_clip_stride,
                                                   int64_t y_step_stride, ScoreBase b1, ScoreBase b2,
                                                   const uint8_t* __restrict__ pix_mask, float thr, FssScales sc, int n, int m,
                                                   int tiles_m, int B, int32_t* __restrict__ partial) {
    constexpr int NW = S + 2;                                  // words of a patch row: counted, I_o, I_s per source
    __shared__ unsigned long long bits[64][NW];
    __shared__ int red[4][2 + S * 8 * 3];
    const int b = blockIdx.y, z = blockIdx.z;
    const int64_t P = (int64_t)n * m;
    const float* out = sg.out[z];
    const int32_t* labels = sg.labels[z] + (int64_t)b * P;
    const int os = sg.out_stride[z];
    const int rows = qt_rows(sg.n_dev[z], sg.N[z]);
    const float* yz = y + z * y_step_stride + b * y_clip_stride;
    const float* f1 = S > 1 ? b1.f + z * b1.step_stride + b * b1.clip_stride : nullptr;
    const float* f2 = S > 2 ? b2.f + z * b2.step_stride + b * b2.clip_stride : nullptr;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = (blockIdx.x / tiles_m) * 32 - 16, c0 = (blockIdx.x % tiles_m) * 32 - 16;      // frame position of patch (0, 0)
    const int gc = c0 + lane;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int pr = w * 16 + i, gr = r0 + pr;
        const bool in = gr >= 0 && gr < n && gc >= 0 && gc < m;
        bool counted = false, io = false, is[S];
#pragma unroll
        for (int s = 0; s < S; ++s) is[s] = false;
        if (in) {
            const int64_t p = (int64_t)gr * m + gc;
            const int lab = labels[p];
            counted = lab >= 0 && lab < rows && !(pix_mask && pix_mask[p]);
            if (counted) {
                io = yz[p] > thr;
                is[0] = out[(int64_t)lab * os] > thr;
                if (S > 1) is[1] = f1[p] > thr;
                if (S > 2) is[2] = f2[p] > thr;
            }
        }
        const unsigned long long wc = __ballot(counted), wo = __ballot(io);
        unsigned long long ws[S];
#pragma unroll
        for (int s = 0; s < S; ++s) ws[s] = __ballot(is[s]);
        if (lane == 0) {
            bits[pr][0] = wc;
            bits[pr][1] = wo;
#pragma unroll
            for (int s = 0; s < S; ++s) bits[pr][2 + s] = ws[s];
        }
    }
    __syncthreads();
    const int cc = (threadIdx.x & 31) + 16, rr = (threadIdx.x >> 5) * 4 + 16;       // patch column, first patch row of the centres
    bool ctr[4], ev[4];
    int nc = 0, ne = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ctr[j] = (bits[rr + j][0] >> cc) & 1;
        ev[j] = (bits[rr + j][1] >> cc) & 1;
        nc += __popcll(__ballot(ctr[j]));
        ne += __popcll(__ballot(ev[j]));
    }
    if (lane == 0) {
        red[w][0] = nc;
        red[w][1] = ne;
    }
    for (int k = 0; k < sc.K; ++k) {
        const int h = sc.h[k];
        const unsigned long long cmask = ((1ull << (2 * h + 1)) - 1) << (cc - h);
        int co[4], cs[S][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            co[j] = 0;
#pragma unroll
            for (int s = 0; s < S; ++s) cs[s][j] = 0;
        }
        for (int i = 0; i < 2 * h + 4; ++i) {                  // patch row rr - h + i is in the window of centre j iff j <= i <= j + 2h
            const unsigned long long* row = bits[rr - h + i];
            const int po = __popcll(row[1] & cmask);
            int ps[S];
#pragma unroll
            for (int s = 0; s < S; ++s) ps[s] = __popcll(row[2 + s] & cmask);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool hit = i >= j && i <= j + 2 * h;
                co[j] += hit ? po : 0;
#pragma unroll
                for (int s = 0; s < S; ++s) cs[s][j] += hit ? ps[s] : 0;
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            int v[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = cs[s][j] - co[j];
                v[0] += ctr[j] ? d * d : 0;
                v[1] += ctr[j] ? cs[s][j] * cs[s][j] : 0;
                v[2] += ctr[j] ? co[j] * co[j] : 0;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
            }
            if (lane == 0) {
                int* r = red[w] + 2 + (s * sc.K + k) * 3;
                r[0] = v[0];
                r[1] = v[1];
                r[2] = v[2];
            }
        }
    }
    __syncthreads();
    auto total = [&](int v) { return (red[0][v] + red[1][v]) + (red[2][v] + red[3][v]); };
    int32_t* dst = partial + (((int64_t)z * B + b) * gridDim.x + blockIdx.x) * (S * sc.K * 5);
    for (int v = threadIdx.x; v < S * sc.K * 5; v += 256) {
        const int slot = v % 5;
        dst[v] = slot < 2 ? total(slot) : total(2 + (v / 5) * 3 + slot - 2);
    }
}

// Ice-edge displacement of a rollout (edge_distance()): k_fss_multi's reads, sources and counting rule, but what is compared
// is where the ice edge lies.  ice(x, p) = counted(p) && x[p] > thr (strict, fp32: NaN and -inf are not ice, +inf is); the edge
// set E(x) holds the ice pixels with a 4-neighbour that is inside the frame, counted and not ice (frame borders and uncounted
// pixels make no edge).  For each source f the eight integers of include/qtmpnn_edges.h are kept per (step, clip, band of 16 rows):
// [|E(f)|, |E(y)|, sum q fo, sum q of, sum d2 fo, sum d2 of, max d2 fo, max d2 of], d2(p, E) = min over e of dr^2 + dc^2,
// q = isqrt(65536 d2), `fo` over p in E(f) against E(y), `of` the reverse; a direction whose target set is empty gives 0.
// The search is over the whole frame: no radius, no cap.
//
// Two launches.  Every query may reach any row of the frame, so a searching workgroup needs the whole frame's edge sets, while
// building them costs a read of every field through the labels.  Building them inside the searching workgroup would repeat
// those reads once per band of the frame (16 times at 256 rows); instead k_edge_planes reads every pixel once (plus one halo
// row on either side of its band) and leaves the edge sets as bit-planes in a small global scratch -- one 64-bit word per 64
// columns of a row, (S + 1) planes of n * ceil(m / 64) words per (step, clip): 32 KB for a 256 x 256 frame with three sources
// -- and k_edge_search loads all of a (step, clip)'s planes into LDS and answers the queries of its band.  The second launch
// follows the first in the stream; the scratch stays in L2.
//
// k_edge_planes: workgroup (band, clip, step).  The band's 16 rows and the row above and below are 18 * W (row, word) units, W =
// ceil(m / 64) <= 4, dealt to the four waves in turn; lane l is column 64 j + l, and a ballot turns `counted` and every field's
// ice into one word (lanes outside the frame are false, so rows and columns beyond it count as "no neighbour").  After a
// barrier a thread forms an edge word of (row, word, field): with N = counted & ~ice, edge = ice & (N above | N below |
// N << 1 | bit 63 of the word to the left | N >> 1 | bit 0 of the word to the right).
//
// k_edge_search: workgroup (band, clip, step), all planes in LDS (at most 4 * 1024 words).  For each source and direction the
// queries are the set bits of the band's rows of one plane.  They are dealt to lanes densely: the band has 16 W <= 64 words,
// lane l of every wave takes the popcount of word l and an inclusive scan over the wave gives every word its offset; wave w
// then visits words w, w + 4, ... and the lanes whose bit is set store (row, column) into an LDS queue at offset + rank (rank =
// popcount of the lower set bits).  After a barrier thread t answers entries t, t + 256, ...: no lane idles on a pixel that is no
// query, and which lane answers which query does not matter to an integer sum.  A query at (r, c) walks the target plane's rows
// r, r -+ 1, r -+ 2, ... and stops once dr^2 >= the best d2 so far or both rows are outside the frame; in a row the nearest set
// bit is found per word with count-leading / trailing-zeros (the word holding c is split at c).  Lanes still diverge in how far
// they walk; a wave is done when its farthest query is.
// q: s = (uint64)sqrt((double)(d2 << 16)), then s is stepped down while s * s > x and up while (s + 1)^2 <= x in 64-bit
// integers, so q is floor(sqrt(65536 d2)) whatever the estimate was.
// Widths (frames of at most 256 x 256, which the launcher enforces): d2 <= 255^2 + 255^2 = 130050, q <= 92321.  A band has at most
// 16 * 256 = 4096 queries per direction, so a thread's, a wave's and a band's sum q <= 4096 * 92321 = 378 146 816 and sum d2 <=
// 4096 * 130050 = 532 684 800, both < 2^31: every partial is a non-negative int32.  A frame's total (16 bands) is not bounded so
// and is the caller's to add in int64.  Reduction: 64-lane butterflies (add, or max for the two max slots), then the four waves.
// Integers, no atomics: the same bits on every run, eager or replayed.
constexpr int EDGE_BAND = 16, EDGE_MAX = 256;

template <int S>
__global__ __launch_bounds__(256) void k_edge_planes(ScoreSeg sg, const float* __restrict__ y, int64_t y_clip_stride,
                                                     int64_t y_step_stride, ScoreBase b1, ScoreBase b2,
                                                     const uint8_t* __restrict__ pix_mask, float thr, int n, int m, int W, int B,
                                                     unsigned long long* __restrict__ planes) {
    constexpr int NF = S + 1;                                  // fields: y, then the sources
    __shared__ unsigned long long bits[EDGE_BAND + 2][4][NF + 1];       // [row][word][counted, ice of y, ice of each source]
    const int b = blockIdx.y, z = blockIdx.z;
    const int64_t P = (int64_t)n * m;
    const float* out = sg.out[z];
    const int32_t* labels = sg.labels[z] + (int64_t)b * P;
    const int os = sg.out_stride[z];
    const int rows = qt_rows(sg.n_dev[z], sg.N[z]);
    const float* yz = y + z * y_step_stride + b * y_clip_stride;
    const float* f1 = S > 1 ? b1.f + z * b1.step_stride + b * b1.clip_stride : nullptr;
    const float* f2 = S > 2 ? b2.f + z * b2.step_stride + b * b2.clip_stride : nullptr;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = blockIdx.x * EDGE_BAND;
    for (int u = w; u < (EDGE_BAND + 2) * W; u += 4) {
        const int i = u / W, j = u - i * W;
        const int gr = r0 - 1 + i, gc = j * 64 + lane;
        bool counted = false, ice[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) ice[f] = false;
        if (gr >= 0 && gr < n && gc < m) {
            const int64_t p = (int64_t)gr * m + gc;
            const int lab = labels[p];
            counted = lab >= 0 && lab < rows && !(pix_mask && pix_mask[p]);
            if (counted) {
                ice[0] = yz[p] > thr;
                ice[1] = out[(int64_t)lab * os] > thr;
                if (S > 1) ice[2] = f1[p] > thr;
                if (S > 2) ice[3] = f2[p] > thr;
            }
        }
        const unsigned long long wc = __ballot(counted);
        unsigned long long wi[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) wi[f] = __ballot(ice[f]);
        if (lane == 0) {
            bits[i][j][0] = wc;
#pragma unroll
            for (int f = 0; f < NF; ++f) bits[i][j][1 + f] = wi[f];
        }
    }
    __syncthreads();
    unsigned long long* dst = planes + ((int64_t)z * B + b) * NF * n * W;
    for (int v = threadIdx.x; v < EDGE_BAND * W * NF; v += 256) {
        const int f = v % NF, u = v / NF;
        const int i = 1 + u / W, j = u % W;
        const int gr = r0 + i - 1;
        if (gr >= n) continue;
        auto open = [&](int ii, int jj) { return bits[ii][jj][0] & ~bits[ii][jj][1 + f]; };       // counted and not ice
        const unsigned long long here = open(i, j);
        unsigned long long nb = open(i - 1, j) | open(i + 1, j) | (here << 1) | (here >> 1);
        if (j > 0) nb |= open(i, j - 1) >> 63;
        if (j + 1 < W) nb |= open(i, j + 1) << 63;
        dst[((int64_t)f * n + gr) * W + j] = bits[i][j][1 + f] & nb;
    }
}

// min |dc| to a set bit of a plane row (W words at `row`) from column c, or 1 << 20 if the row is empty
__device__ __forceinline__ int edge_row_dist(const unsigned long long* row, int W, int c) {
    const int wc = c >> 6, bit = c & 63;
    int bd = 1 << 20;
    for (int j = 0; j < W; ++j) {
        const unsigned long long x = row[j];
        if (!x) continue;
        if (j < wc) bd = min(bd, c - (j * 64 + 63 - __builtin_clzll(x)));
        else if (j > wc) bd = min(bd, j * 64 + __builtin_ctzll(x) - c);
        else {
            const unsigned long long lo = x & (~0ull >> (63 - bit)), hi = x & (~0ull << bit);
            if (lo) bd = min(bd, bit - (63 - __builtin_clzll(lo)));
            if (hi) bd = min(bd, __builtin_ctzll(hi) - bit);
        }
    }
    return bd;
}

template <int S>
__global__ __launch_bounds__(256) void k_edge_search(const unsigned long long* __restrict__ planes, int n, int W, int B,
                                                     int32_t* __restrict__ partial) {
    constexpr int NF = S + 1;
    __shared__ unsigned long long pl[NF * 4 * EDGE_MAX];      // [field][row][word], n * W <= 4 * EDGE_MAX words each
    __shared__ unsigned short queue[EDGE_BAND * EDGE_MAX];     // (local row << 8) | column
    __shared__ int some[NF];                                   // the field's edge set is not empty
    __shared__ int red[4][S * 8];
    const int b = blockIdx.y, z = blockIdx.z;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = blockIdx.x * EDGE_BAND, nr = min(EDGE_BAND, n - r0);
    const int words = n * W;
    const unsigned long long* src = planes + ((int64_t)z * B + b) * NF * words;
    if (threadIdx.x < NF) some[threadIdx.x] = 0;
    __syncthreads();
    for (int f = 0; f < NF; ++f) {
        unsigned long long any = 0;
        for (int v = threadIdx.x; v < words; v += 256) {
            const unsigned long long x = src[f * words + v];
            pl[f * words + v] = x;
            any |= x;
        }
        if (any) some[f] = 1;                                  // every writer stores the same value
    }
    __syncthreads();
    const int bw = nr * W;                                     // words of the band's rows of one plane, <= 64
    for (int s = 0; s < S; ++s) {
        int res[8];
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            // dir 0 (fo): queries E(f_s), target E(y); dir 1 (of): queries E(y), target E(f_s)
            const unsigned long long* qp = pl + (dir == 0 ? 1 + s : 0) * words + r0 * W;
            const unsigned long long* tp = pl + (dir == 0 ? 0 : 1 + s) * words;
            const bool target = some[dir == 0 ? 0 : 1 + s] != 0;
            int cnt = lane < bw ? __popcll(qp[lane]) : 0, incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            const int total = __shfl(incl, 63, 64);
            res[dir] = total;                                  // |E(f_s)|, |E(y)| of the band
            int sq = 0, sd = 0, mx = 0;
            if (target && total) {                             // uniform over the workgroup
                for (int u = w; u < bw; u += 4) {
                    const int base = __shfl(incl - cnt, u, 64);
                    const unsigned long long x = qp[u];
                    if ((x >> lane) & 1) {
                        const int rank = __popcll(x & ((1ull << lane) - 1));
                        queue[base + rank] = (unsigned short)(((u / W) << 8) | ((u % W) * 64 + lane));
                    }
                }
                __syncthreads();
                for (int e = threadIdx.x; e < total; e += 256) {
                    const int r = r0 + (queue[e] >> 8), c = queue[e] & 255;
                    int best = 0x7fffffff;
                    for (int k = 0; k < n; ++k) {
                        const int k2 = k * k;
                        if (k2 >= best) break;
                        const int lo = r - k, hi = r + k;
                        if (lo < 0 && hi >= n) break;
                        if (lo >= 0) {
                            const int d = edge_row_dist(tp + lo * W, W, c);
                            if (d < (1 << 20)) best = min(best, k2 + d * d);
                        }
                        if (k > 0 && hi < n) {
                            const int d = edge_row_dist(tp + hi * W, W, c);
                            if (d < (1 << 20)) best = min(best, k2 + d * d);
                        }
                    }
                    const unsigned long long x = (unsigned long long)best << 16;
                    unsigned long long q = (unsigned long long)sqrt((double)x);
                    while (q * q > x) --q;
                    while ((q + 1) * (q + 1) <= x) ++q;
                    sq += (int)q;
                    sd += best;
                    mx = max(mx, best);
                }
                __syncthreads();                               // the queue is rewritten by the next direction
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sq += __shfl_xor(sq, d, 64);
                sd += __shfl_xor(sd, d, 64);
                mx = max(mx, __shfl_xor(mx, d, 64));
            }
            res[2 + dir] = sq;
            res[4 + dir] = sd;
            res[6 + dir] = mx;
        }
        if (lane == 0) {
#pragma unroll
            for (int v = 0; v < 8; ++v) red[w][s * 8 + v] = res[v];
        }
    }
    __syncthreads();
    int32_t* dst = partial + (((int64_t)z * B + b) * gridDim.x + blockIdx.x) * (S * 8);
    if (threadIdx.x < S * 8) {
        const int v = threadIdx.x, slot = v & 7;
        if (slot < 2) dst[v] = red[0][v];                      // every wave counted the whole band
        else if (slot < 6) dst[v] = (red[0][v] + red[1][v]) + (red[2][v] + red[3][v]);
        else dst[v] = max(max(red[0][v], red[1][v]), max(red[2][v], red[3][v]));
    }
}

// Per-pixel verification sums: k_score_multi's reads and counting rule, kept per pixel and summed over the clips instead of
// per clip and summed over the pixels.  One thread owns pixel p of step z and is the only writer of its 8 * S running doubles
// (maps + z * maps_step_stride, laid out (S, 8, P)): it loads the three sums of every source, adds the clips' terms to them
// one by one in clip order in double, and stores them; the class counts are integers (exact in any order) and are added to
// their running values at the end.  d = f - y is formed in fp32 as in k_score_multi and then widened; d * d of a widened fp32
// is exact in double, so contracting it into the add changes no bit.  The result is the left-to-right float64 sum over every
// clip that was ever added, however the clips were batched.  No atomics, no LDS, no cross-thread step; launches that share
// `maps` are ordered by their stream.
template <int S>
__global__ __launch_bounds__(256) void k_score_maps(ScoreSeg sg, const float* __restrict__ y, int64_t y_clip_stride,
                                                    int64_t y_step_stride, ScoreBase b1, ScoreBase b2,
                                                    const uint8_t* __restrict__ pix_mask, float thr, int64_t P, int B,
                                                    double* __restrict__ maps, int64_t maps_step_stride) {
    const int z = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || (pix_mask && pix_mask[p])) return;         // a masked pixel counts in no clip: its doubles stay as they are
    const float* out = sg.out[z];
    const int32_t* labels = sg.labels[z] + p;
    const int os = sg.out_stride[z];
    const int rows = qt_rows(sg.n_dev[z], sg.N[z]);
    const float* yz = y + z * y_step_stride + p;
    const float* f1 = S > 1 ? b1.f + z * b1.step_stride + p : nullptr;
    const float* f2 = S > 2 ? b2.f + z * b2.step_stride + p : nullptr;
    double* mz = maps + z * maps_step_stride + p;             // slot k of source s: mz[(s * 8 + k) * P]
    double sum[S][3];
    int cls[S][3], n = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sum[s][k] = mz[(s * 8 + 1 + k) * P];
            cls[s][k] = 0;
        }
    }
    for (int b = 0; b < B; ++b) {
        const int lab = labels[b * P];
        if (lab < 0 || lab >= rows) continue;
        const float t = yz[b * y_clip_stride];
        const bool ty = t > thr;
        float f[S];
        f[0] = out[(int64_t)lab * os];
        if (S > 1) f[1] = f1[b * b1.clip_stride];
        if (S > 2) f[2] = f2[b * b2.clip_stride];
        ++n;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float d32 = f[s] - t;
            const double d = (double)d32;
            const bool tf = f[s] > thr;
            sum[s][0] += d;
            sum[s][1] += fabs(d);
            sum[s][2] += d * d;
            cls[s][0] += (tf && ty) ? 1 : 0;
            cls[s][1] += (tf && !ty) ? 1 : 0;
            cls[s][2] += (!tf && ty) ? 1 : 0;
        }
    }
    if (n == 0) return;                                       // no clip of this launch has a node here: nothing to add
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double* m = mz + (int64_t)s * 8 * P;
        m[0] += (double)n;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            m[(1 + k) * P] = sum[s][k];
            m[(4 + k) * P] += (double)cls[s][k];
        }
        m[7 * P] += (double)(n - cls[s][0] - cls[s][1] - cls[s][2]);
    }
}

// Event dates of a rollout (break-up / freeze-up): the first output step from which a pixel stays in the target state g for k
// consecutive steps, per source (observed, model, optionally one dense field).  k_score_maps' reads and counting rule, but along
// the time axis: one thread owns pixel p of clip b, reads its label once per step and serves every source from it, and carries
// per source the current run length and the date in registers over the chunk's steps.  A launch with z0 == 0 initialises the
// state (date -2 under the mask, else -1; run 0, or -1 where the launch frame is already in the target state: such a pixel has
// no event, and a negative run is never advanced), a launch with z0 > 0 loads what the previous chunk stored.  A pixel without
// a valid node at any step ends as -2 for every source.  No atomics, no LDS, no cross-thread step; chunks are ordered by their
// stream.
template <int S1>
__global__ __launch_bounds__(256) void k_event_scan(ScoreSeg sg, int nseg, const float* __restrict__ y, int64_t y_clip_stride,
                                                    int64_t y_step_stride, ScoreBase b1, const uint8_t* __restrict__ pix_mask,
                                                    const float* __restrict__ launch, int64_t launch_clip_stride, float thr,
                                                    int target, int k, int z0, int64_t P, int32_t* __restrict__ dates,
                                                    int32_t* __restrict__ runs) {
    const int b = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const bool g = target != 0;
    const int64_t st = ((int64_t)b * S1) * P + p;             // source s of this pixel: st + s * P
    int date[S1], run[S1];
    if (z0 == 0) {
        const int d0 = (pix_mask && pix_mask[p]) ? -2 : -1;
        const int r0 = ((launch[b * launch_clip_stride + p] > thr) == g) ? -1 : 0;
#pragma unroll
        for (int s = 0; s < S1; ++s) {
            date[s] = d0;
            run[s] = r0;
        }
    } else {
#pragma unroll
        for (int s = 0; s < S1; ++s) {
            date[s] = dates[st + s * P];
            run[s] = runs[st + s * P];
        }
    }
    bool dead = date[0] == -2;                                // masked, or without a node at an earlier step
    const float* yp = y + b * y_clip_stride + p;
    const float* fp = S1 > 2 ? b1.f + b * b1.clip_stride + p : nullptr;
    for (int z = 0; z < nseg && !dead; ++z) {
        const int lab = sg.labels[z][(int64_t)b * P + p];
        if (lab < 0 || lab >= qt_rows(sg.n_dev[z], sg.N[z])) {
            dead = true;
            break;
        }
        float f[S1];
        f[0] = yp[z * y_step_stride];
        f[1] = sg.out[z][(int64_t)lab * sg.out_stride[z]];
        if (S1 > 2) f[2] = fp[z * b1.step_stride];
#pragma unroll
        for (int s = 0; s < S1; ++s) {
            if (run[s] < 0) continue;
            run[s] = ((f[s] > thr) == g) ? run[s] + 1 : 0;
            if (run[s] >= k && date[s] == -1) date[s] = z0 + z - k + 1;
        }
    }
#pragma unroll
    for (int s = 0; s < S1; ++s) {
        dates[st + s * P] = dead ? -2 : date[s];
        runs[st + s * P] = run[s];
    }
}

// The eight sums of the date errors per (clip, forecast source): one workgroup each, every thread over its pixels in pixel
// order in int64, then 64-lane butterflies and (w0 + w1) + (w2 + w3).  Integers: exact in any order.
__global__ __launch_bounds__(256) void k_event_sums(const int32_t* __restrict__ dates, int S1, int64_t P,
                                                    int64_t* __restrict__ sums) {
    __shared__ long long red[4][8];
    const int b = blockIdx.x, s = 1 + blockIdx.y;             // source 0 is the observed one
    const int32_t* dob = dates + ((int64_t)b * S1) * P;
    const int32_t* dfc = dob + (int64_t)s * P;
    long long acc[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = 0;
    for (int64_t p = threadIdx.x; p < P; p += 256) {
        const int o = dob[p], f = dfc[p];
        if (o == -2) continue;
        acc[0] += 1;
        if (o >= 0 && f >= 0) {
            const long long e = (long long)f - o;
            acc[1] += e;
            acc[2] += e < 0 ? -e : e;
            acc[3] += e * e;
            acc[4] += 1;
        } else if (f >= 0) {
            acc[5] += 1;
        } else if (o >= 0) {
            acc[6] += 1;
        } else {
            acc[7] += 1;
        }
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[v] += __shfl_xor(acc[v], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int v = 0; v < 8; ++v) red[threadIdx.x >> 6][v] = acc[v];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int v = threadIdx.x;
        sums[((int64_t)b * (S1 - 1) + (s - 1)) * 8 + v] = (int64_t)((red[0][v] + red[1][v]) + (red[2][v] + red[3][v]));
    }
}

// What the six rollout launchers have in common: the segment arrays of 1..16 steps into `sg`, and the dense baseline fields
// that are present, in order, into `bs` (`nb` of them: the kernels are instantiated per source count).  Returns the reason of a
// refusal, or null; the entry reports it under its own name (QT_ARG).
struct ScoreSetup {
    ScoreSeg sg;
    ScoreBase bs[2];
    int nb;
};

const char* score_setup(ScoreSetup& st, int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                        const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride, int64_t y_step_stride,
                        ScoreBase base1, ScoreBase base2) {
    if (!(nseg >= 1 && nseg <= 16)) return "nseg must be 1..16";
    if (!(outs && out_strides && labels && Ns && n_devs && y)) return "null pointer";
    if (!(y_clip_stride >= 0 && y_step_stride >= 0 && base1.clip_stride >= 0 && base1.step_stride >= 0 &&
          base2.clip_stride >= 0 && base2.step_stride >= 0))
        return "negative stride";
    st = {};
    ScoreSeg& sg = st.sg;
    for (int z = 0; z < nseg; ++z) {
        if (!(labels[z] && Ns[z] >= 0 && (outs[z] || Ns[z] == 0) && out_strides[z] >= 1)) return "bad segment";
        sg.out[z] = outs[z]; sg.out_stride[z] = out_strides[z]; sg.labels[z] = labels[z]; sg.N[z] = Ns[z]; sg.n_dev[z] = n_devs[z];
    }
    if (base1.f) st.bs[st.nb++] = base1;
    if (base2.f) st.bs[st.nb++] = base2;
    return nullptr;
}

}  // namespace

extern "C" int qt_score_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                                const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                                int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                                const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                                const uint8_t* pix_mask, float thr, int B, int n, int m, float* partial, void* stream) {
    ScoreSetup st;
    const char* why = score_setup(st, nseg, outs, out_strides, labels, Ns, n_devs, y, y_clip_stride, y_step_stride,
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride});
    QT_ARG(!why, why);
    QT_ARG(partial, "null pointer");
    QT_ARG(B > 0 && B <= 65535 && n > 0 && m > 0, "bad sizes");
    const int64_t P = (int64_t)n * m;
    const dim3 grid(qt_cdiv(P, 1024), B, nseg);
    // the kernel's partial rows are sized for the sources present
    auto k = st.nb == 0 ? k_score_multi<1> : st.nb == 1 ? k_score_multi<2> : k_score_multi<3>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, st.sg, y, y_clip_stride, y_step_stride, st.bs[0], st.bs[1],
                       pix_mask, thr, P, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_reliability_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                                      const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                                      int64_t y_step_stride, const float* base1, int64_t base1_clip_stride,
                                      int64_t base1_step_stride, const float* base2, int64_t base2_clip_stride,
                                      int64_t base2_step_stride, const uint8_t* pix_mask, float thr, int B, int n, int m,
                                      int bins, float* partial, void* stream) {
    ScoreSetup st;
    const char* why = score_setup(st, nseg, outs, out_strides, labels, Ns, n_devs, y, y_clip_stride, y_step_stride,
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride});
    QT_ARG(!why, why);
    QT_ARG(bins >= 2 && bins <= 32, "bins must be 2..32");
    QT_ARG(partial, "null partial");
    QT_ARG(B > 0 && B <= 65535 && n > 0 && m > 0, "bad sizes");
    const int64_t P = (int64_t)n * m;
    const dim3 grid(qt_cdiv(P, 1024), B, nseg);
    auto k = st.nb == 0 ? k_reliability_multi<1> : st.nb == 1 ? k_reliability_multi<2> : k_reliability_multi<3>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, st.sg, y, y_clip_stride, y_step_stride, st.bs[0], st.bs[1],
                       pix_mask, thr, bins, P, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_fss_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                              const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                              int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                              const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                              const uint8_t* pix_mask, float thr, int B, int n, int m, int nscales, const int* scales,
                              int32_t* partial, void* stream) {
    ScoreSetup st;
    const char* why = score_setup(st, nseg, outs, out_strides, labels, Ns, n_devs, y, y_clip_stride, y_step_stride,
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride});
    QT_ARG(!why, why);
    QT_ARG(nscales >= 1 && nscales <= 8, "nscales must be 1..8");
    QT_ARG(scales, "null scales");
    FssScales sc = {};
    sc.K = nscales;
    for (int k = 0; k < nscales; ++k) {
        // the kernel's column mask and halo hold windows up to 33 wide and no wider
        QT_ARG(scales[k] >= 1 && scales[k] <= 33 && (scales[k] & 1), "scales must be odd and in 1..33");
        QT_ARG(k == 0 || scales[k] > scales[k - 1], "scales must be strictly increasing");
        sc.h[k] = scales[k] / 2;
    }
    QT_ARG(partial, "null partial");
    QT_ARG(B > 0 && B <= 65535 && n > 0 && m > 0, "bad sizes");
    const int tiles_m = qt_cdiv(m, 32);
    const int64_t ntile = (int64_t)qt_cdiv(n, 32) * tiles_m;
    QT_ARG(ntile <= 0x7fffffff, "bad sizes");
    const dim3 grid((unsigned)ntile, B, nseg);
    auto k = st.nb == 0 ? k_fss_multi<1> : st.nb == 1 ? k_fss_multi<2> : k_fss_multi<3>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, st.sg, y, y_clip_stride, y_step_stride, st.bs[0], st.bs[1],
                       pix_mask, thr, sc, n, m, tiles_m, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_edge_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                               const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                               int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                               const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                               const uint8_t* pix_mask, float thr, int B, int n, int m, uint64_t* planes, int32_t* partial,
                               void* stream) {
    ScoreSetup st;
    const char* why = score_setup(st, nseg, outs, out_strides, labels, Ns, n_devs, y, y_clip_stride, y_step_stride,
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride});
    QT_ARG(!why, why);
    QT_ARG(planes && partial, "null planes / partial");
    QT_ARG(B > 0 && B <= 65535 && n > 0 && m > 0, "bad sizes");
    // k_edge_search holds a (step, clip)'s planes in LDS and packs a query into 16 bits; its int32 sums are proved for this size
    QT_ARG(n <= EDGE_MAX && m <= EDGE_MAX, "frame larger than 256 x 256");
    const int W = qt_cdiv(m, 64);
    const dim3 grid(qt_cdiv(n, EDGE_BAND), B, nseg);
    auto kp = st.nb == 0 ? k_edge_planes<1> : st.nb == 1 ? k_edge_planes<2> : k_edge_planes<3>;
    auto ks = st.nb == 0 ? k_edge_search<1> : st.nb == 1 ? k_edge_search<2> : k_edge_search<3>;
    hipLaunchKernelGGL(kp, grid, dim3(256), 0, (hipStream_t)stream, st.sg, y, y_clip_stride, y_step_stride, st.bs[0], st.bs[1],
                       pix_mask, thr, n, m, W, B, (unsigned long long*)planes);
    QT_LAUNCHED();
    hipLaunchKernelGGL(ks, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)planes, n, W, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_score_maps(int nseg,const float* const* outs, const int* out_strides, const int32_t* const* labels,
                             const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                             int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                             const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                             const uint8_t* pix_mask, float thr, int B, int n, int m, double* maps, int64_t maps_step_stride,
                             void* stream) {
    ScoreSetup st;
    const char* why = score_setup(st, nseg, outs, out_strides, labels, Ns, n_devs, y, y_clip_stride, y_step_stride,
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride});
    QT_ARG(!why, why);
    QT_ARG(maps, "null pointer");
    QT_ARG(B > 0 && n > 0 && m > 0, "bad sizes");
    const int64_t P = (int64_t)n * m;
    // a step's (S, 8, P) block must fit its stride, or step z would write into step z + 1
    QT_ARG(maps_step_stride >= (int64_t)(1 + st.nb) * 8 * P, "maps_step_stride is smaller than S*8*n*m");
    auto k = st.nb == 0 ? k_score_maps<1> : st.nb == 1 ? k_score_maps<2> : k_score_maps<3>;
    hipLaunchKernelGGL(k, dim3(qt_cdiv(P, 256), nseg), dim3(256), 0, (hipStream_t)stream, st.sg, y, y_clip_stride, y_step_stride,
                       st.bs[0], st.bs[1], pix_mask, thr, P, B, maps, maps_step_stride);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_event_scan(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                             const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                             int64_t y_step_stride, const float* base, int64_t base_clip_stride, int64_t base_step_stride,
                             const uint8_t* pix_mask, float thr, int B, int n, int m, const float* launch,
                             int64_t launch_clip_stride, int target, int k, int z0, int32_t* dates, int32_t* runs,
                             void* stream) {
    ScoreSetup st;
    const char* why = score_setup(st, nseg, outs, out_strides, labels, Ns, n_devs, y, y_clip_stride, y_step_stride,
                                  {base, base_clip_stride, base_step_stride}, {});
    QT_ARG(!why, why);
    QT_ARG(launch, "null pointer");
    QT_ARG(dates && runs, "null dates / runs");
    QT_ARG(B > 0 && B <= 65535 && n > 0 && m > 0, "bad sizes");
    QT_ARG(launch_clip_stride >= 0, "negative stride");
    QT_ARG(target == 0 || target == 1, "target must be 0 (no ice: break-up) or 1 (ice: freeze-up)");
    QT_ARG(k >= 1, "k (persist) must be >= 1");
    QT_ARG(z0 >= 0, "z0 must be >= 0");
    const int64_t P = (int64_t)n * m;
    auto kern = st.nb ? k_event_scan<3> : k_event_scan<2>;
    hipLaunchKernelGGL(kern, dim3(qt_cdiv(P, 256), B), dim3(256), 0, (hipStream_t)stream, st.sg, nseg, y, y_clip_stride,
                       y_step_stride, st.bs[0], pix_mask, launch, launch_clip_stride, thr, target, k, z0, P, dates, runs);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_event_sums(const int32_t* dates, int S1, int B, int n, int m, int64_t* sums, void* stream) {
    QT_ARG(dates && sums, "null dates / sums");
    QT_ARG(S1 == 2 || S1 == 3, "S1 must be 2 or 3");
    QT_ARG(B > 0 && B <= 65535 && n > 0 && m > 0, "bad sizes");
    hipLaunchKernelGGL(k_event_sums, dim3(B, S1 - 1), dim3(256), 0, (hipStream_t)stream, dates, S1, (int64_t)n * m, sums);
    QT_LAUNCHED();
    return QT_OK;
}
