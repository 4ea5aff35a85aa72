// Verification of a rollout, computed where the rollout's outputs are: the per-lead-time sums of score()
// (k_score_multi), the per-pixel maps of score_maps() (k_score_maps), the break-up / freeze-up dates of
// event_dates() with the sums of their errors (k_event_scan, k_event_sums), the per-bin probability sums of
// reliability() (k_reliability_multi), the neighbourhood sums of fss() (k_fss_multi), the ice-edge distances of
// edge_distance() (k_edge_planes, k_edge_search) and the regional area sums of extent() (k_extent_multi).  All of them read the
// head's node values through every step's labels (no
// frame is built) and none has a gradient.  What they share is written once: ScoreArgs, the by-value kernel argument that the
// rollout launchers fill in one host-side setup (score_setup); PixelReader, which says which pixels count and how a
// pixel's values are read; wave_sum / wave_max, the 64-lane butterflies.  A further product is a kernel body over the reader
// and an entry.  The training loss (k_sse, k_loss_multi, k_pool_targets) is in transfer.hip.
#include "qt_common.h"

namespace {

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
// What every rollout kernel is given, by value (about 600 bytes of kernel arguments), followed by the kernel's own extras.
struct ScoreArgs {
    ScoreSeg sg;
    ScoreBase y;                  // the truth
    ScoreBase bs[2];              // the dense baseline fields that are present, in order
    int nb;                       // how many: the kernels are instantiated per source count S = 1 + nb
    const uint8_t* pix_mask;      // (P) or null: a non-zero byte takes the pixel out of every clip and step
    float thr;
    __device__ bool masked(int64_t p) const { return pix_mask && pix_mask[p]; }
};

// The pixels of step z of clip b as every product reads them.  A pixel p COUNTS iff its label is a node of the step (0 <= lab <
// rows, rows = the step's node count on the device capped by its capacity) and the pixel mask does not cover it: counted().
// An uncounted pixel is read no further and adds nothing anywhere.  A counted pixel has the truth y[p] and S sources: the
// model's node value through the label, then the dense fields at p (load(): in that order).  A kernel that walks the clips at
// a fixed pixel constructs the reader at clip 0 and steps it with next_clip(); one that walks the steps constructs one per step.
template <int S>
struct PixelReader {
    const ScoreArgs& a;
    const int64_t P;
    const float* out;             // node values of the step
    const int32_t* labels;
    const float *yz, *dense[2];
    int os, rows;
    __device__ PixelReader(const ScoreArgs& a, int64_t P, int b, int z)
        : a(a), P(P), out(a.sg.out[z]), labels(a.sg.labels[z] + (int64_t)b * P),
          yz(a.y.f + z * a.y.step_stride + b * a.y.clip_stride), os(a.sg.out_stride[z]), rows(qt_rows(a.sg.n_dev[z], a.sg.N[z])) {
#pragma unroll
        for (int s = 1; s < S; ++s) dense[s - 1] = a.bs[s - 1].f + z * a.bs[s - 1].step_stride + b * a.bs[s - 1].clip_stride;
    }
    __device__ void next_clip() {
        labels += P;
        yz += a.y.clip_stride;
#pragma unroll
        for (int s = 1; s < S; ++s) dense[s - 1] += a.bs[s - 1].clip_stride;
    }
    __device__ int label(int64_t p) const { return labels[p]; }
    __device__ bool node(int lab) const { return lab >= 0 && lab < rows; }
    __device__ bool counted(int64_t p, int lab) const { return node(lab) && !a.masked(p); }
    __device__ float truth(int64_t p) const { return yz[p]; }
    __device__ void load(int64_t p, int lab, float* f) const {
        f[0] = out[(int64_t)lab * os];
#pragma unroll
        for (int s = 1; s < S; ++s) f[s] = dense[s - 1][p];
    }
    // The wave's 64 pixels (this lane's is p, or none if !in) as S + 2 ballot words: counted, then ice = counted && value > thr
    // (strict, fp32: a NaN is not ice) of the truth and of every source
    __device__ void ice_words(bool in, int64_t p, unsigned long long* w) const {
        bool c = false, ice[S + 1];
#pragma unroll
        for (int s = 0; s <= S; ++s) ice[s] = false;
        if (in) {
            const int lab = label(p);
            c = counted(p, lab);
            if (c) {
                float f[S];
                ice[0] = truth(p) > a.thr;
                load(p, lab, f);
#pragma unroll
                for (int s = 0; s < S; ++s) ice[1 + s] = f[s] > a.thr;
            }
        }
        w[0] = __ballot(c);
#pragma unroll
        for (int s = 0; s <= S; ++s) w[1 + s] = __ballot(ice[s]);
    }
};

// Sum / maximum over the 64 lanes of a wave, left in every lane: the butterfly xor 32, 16, 8, 4, 2, 1, in that order (for a
// float sum the order is part of the result).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// Forecast verification of a rollout: the reader's pixels, summed per (step, clip, tile of 1024 pixels) and per source.
// Per tile: n, then per source [sum d, sum |d|, sum d^2, hits, over, under]; the correct negatives are n - hits - over - under
// (every counted pixel falls in exactly one of the four classes, and the counts are integers <= 1024: exact in fp32).
template <int S>
__global__ __launch_bounds__(256) void k_score_multi(ScoreArgs a, int64_t P, int B, float* __restrict__ partial) {
    constexpr int NV = 1 + 6 * S;
    __shared__ float red[4][NV];
    const int b = blockIdx.y, z = blockIdx.z;
    const PixelReader<S> rd(a, P, b, z);
    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t p = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (p >= P) continue;
        const int lab = rd.label(p);
        if (!rd.counted(p, lab)) continue;
        const float t = rd.truth(p);
        const bool ty = t > a.thr;
        float f[S];
        rd.load(p, lab, f);
        acc[0] += 1.0f;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float* as = acc + 1 + 6 * s;
            const float d = f[s] - t;
            const bool tf = f[s] > a.thr;
            as[0] += d;
            as[1] += fabsf(d);
            as[2] += d * d;
            as[3] += (tf && ty) ? 1.0f : 0.0f;
            as[4] += (tf && !ty) ? 1.0f : 0.0f;
            as[5] += (!tf && ty) ? 1.0f : 0.0f;
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = wave_sum(acc[v]);
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

// Probability verification of a rollout: k_score_multi's reads (PixelReader) and tile shape, with the forecast value
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
__global__ __launch_bounds__(256) void k_reliability_multi(ScoreArgs a, int K, int64_t P, int B, float* __restrict__ partial) {
    __shared__ float red[4][S * 32 * 4];
    const int b = blockIdx.y, z = blockIdx.z;
    const PixelReader<S> rd(a, P, b, z);
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
            lab = rd.label(p);
            counted = rd.counted(p, lab);
        }
        ev[j] = false;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            f[s][j] = 0.0f;
            e2[s][j] = 0.0f;
            bin[s][j] = -1;
        }
        if (!counted) continue;
        ev[j] = rd.truth(p) > a.thr;
        const float o = ev[j] ? 1.0f : 0.0f;
        float v[S];
        rd.load(p, lab, v);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            f[s][j] = v[s];
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
                sf = wave_sum(sf);
                sq = wave_sum(sq);
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

// Regional ice extent, ice area and the over- / under-forecast areas of a rollout (extent(); slot table in
// include/qtmpnn.h, qt_extent_rollout): k_score_multi's reads (PixelReader) and tile shape, with two per-pixel maps shared by all clips and
// steps: region[p] (int8; 0 <= r < R places the pixel in region r, any other value in none: such a pixel is read no further and
// adds nothing; null: every pixel is in region 0) and area[p] (the pixel's weight a; null: 1).  With I_o = y > thr and I_s =
// f_s > thr (strict, fp32) every (region, tile) keeps row 0 [n, A = sum a, E_o = sum a I_o, SIA_o = sum a y] and per source
// row 1 + s [E_s = sum a I_s, SIA_s = sum a f_s, O_s = sum a I_s (1 - I_o), U_s = sum a (1 - I_s) I_o] over its counted pixels.
// k_reliability_multi's order: every thread keeps its four pixels' region, a, a * y, a * f_s (one fp32 rounding each) and
// indicators in registers and the workgroup walks the regions; for region r a lane adds the terms of its pixels that lie in r
// and +0 for the others, its pixels p, p + 256, p + 512, p + 768 of the tile in that order (starting from +0), then the 64-lane
// butterfly (xor 32, 16, 8, 4, 2, 1), then (w0 + w1) + (w2 + w3) over the four waves.  A wave none of whose pixels is in the
// region skips its butterflies: every lane holds +0 there, which is what they would leave.  n is a popcount of wave ballots.  A
// term is selected, never multiplied by an indicator, so a NaN stays where it is: a NaN forecast is not ice (it is `under`
// where the truth is ice) and makes SIA_s of its own region, tile and source NaN and nothing else; a NaN truth likewise SIA_o.
// No atomics: the same bits on every run, eager or replayed.  LDS: 4 waves x R <= 32 regions x (1 + S) <= 4 rows x 4 floats <= 8 KB.
template <int S>
__global__ __launch_bounds__(256) void k_extent_multi(ScoreArgs a, const int8_t* __restrict__ region,
                                                      const float* __restrict__ area, int R, int64_t P, int B,
                                                      float* __restrict__ partial) {
    constexpr int NR = 1 + S;
    __shared__ float red[4][32 * NR * 4];
    const int b = blockIdx.y, z = blockIdx.z;
    const PixelReader<S> rd(a, P, b, z);
    int reg[4];                   // -1: the pixel is not counted or in no region, and matches none
    float w[4], wy[4], wf[S][4];
    bool io[4], is[S][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = (int64_t)blockIdx.x * 1024 + j * 256 + threadIdx.x;
        reg[j] = -1;
        w[j] = 0.0f;
        wy[j] = 0.0f;
        io[j] = false;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            wf[s][j] = 0.0f;
            is[s][j] = false;
        }
        if (p >= P) continue;
        const int r = region ? (int)region[p] : 0;
        if (!(r >= 0 && r < R)) continue;
        const int lab = rd.label(p);
        if (!rd.counted(p, lab)) continue;
        reg[j] = r;
        w[j] = area ? area[p] : 1.0f;
        const float t = rd.truth(p);
        float f[S];
        rd.load(p, lab, f);
        io[j] = t > a.thr;
        wy[j] = __fmul_rn(w[j], t);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            is[s][j] = f[s] > a.thr;
            wf[s][j] = __fmul_rn(w[j], f[s]);
        }
    }
    const int wv = threadIdx.x >> 6;
    for (int r = 0; r < R; ++r) {
        int n = 0;
        float v[NR * 4];
#pragma unroll
        for (int q = 0; q < NR * 4; ++q) v[q] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = reg[j] == r;
            n += __popcll(__ballot(in));
            v[1] += in ? w[j] : 0.0f;
            v[2] += in && io[j] ? w[j] : 0.0f;
            v[3] += in ? wy[j] : 0.0f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                float* vs = v + 4 * (1 + s);
                vs[0] += in && is[s][j] ? w[j] : 0.0f;
                vs[1] += in ? wf[s][j] : 0.0f;
                vs[2] += in && is[s][j] && !io[j] ? w[j] : 0.0f;
                vs[3] += in && !is[s][j] && io[j] ? w[j] : 0.0f;
            }
        }
        if (n) {                  // wave-uniform: n comes from ballots
#pragma unroll
            for (int q = 1; q < NR * 4; ++q) v[q] = wave_sum(v[q]);
        }
        v[0] = (float)n;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < NR * 4; ++q) red[wv][r * NR * 4 + q] = v[q];
        }
    }
    __syncthreads();
    float* dst = partial + (((int64_t)z * B + b) * gridDim.x + blockIdx.x) * ((int64_t)R * NR * 4);
    for (int q = threadIdx.x; q < R * NR * 4; q += 256) dst[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
}

// Neighbourhood verification of a rollout (Fractions Skill Score): k_score_multi's reads (PixelReader), but a
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
__global__ __launch_bounds__(256) void k_fss_multi(ScoreArgs a, FssScales sc, int n, int m, int tiles_m, int B,
                                                   int32_t* __restrict__ partial) {
    constexpr int NW = S + 2;                                  // words of a patch row: counted, I_o, I_s per source
    __shared__ unsigned long long bits[64][NW];
    __shared__ int red[4][2 + S * 8 * 3];
    const int b = blockIdx.y, z = blockIdx.z;
    const PixelReader<S> rd(a, (int64_t)n * m, b, z);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = (blockIdx.x / tiles_m) * 32 - 16, c0 = (blockIdx.x % tiles_m) * 32 - 16;      // frame position of patch (0, 0)
    const int gc = c0 + lane;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        const int pr = w * 16 + i, gr = r0 + pr;
        unsigned long long w[NW];
        rd.ice_words(gr >= 0 && gr < n && gc >= 0 && gc < m, (int64_t)gr * m + gc, w);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NW; ++q) bits[pr][q] = w[q];
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
            for (int q = 0; q < 3; ++q) v[q] = wave_sum(v[q]);
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

// Ice-edge displacement of a rollout (edge_distance()): k_fss_multi's reads (PixelReader), but what is compared
// is where the ice edge lies.  ice(x, p) = counted(p) && x[p] > thr (strict, fp32: NaN and -inf are not ice, +inf is); the edge
// set E(x) holds the ice pixels with a 4-neighbour that is inside the frame, counted and not ice (frame borders and uncounted
// pixels make no edge).  For each source f the eight integers of qt_edge_rollout (include/qtmpnn.h) are kept per (step, clip, band of 16 rows):
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
__global__ __launch_bounds__(256) void k_edge_planes(ScoreArgs a, int n, int m, int W, int B,
                                                     unsigned long long* __restrict__ planes) {
    constexpr int NF = S + 1;                                  // fields: y, then the sources
    __shared__ unsigned long long bits[EDGE_BAND + 2][4][NF + 1];       // [row][word][counted, ice of y, ice of each source]
    const int b = blockIdx.y, z = blockIdx.z;
    const PixelReader<S> rd(a, (int64_t)n * m, b, z);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = blockIdx.x * EDGE_BAND;
    for (int u = w; u < (EDGE_BAND + 2) * W; u += 4) {
        const int i = u / W, j = u - i * W;
        const int gr = r0 - 1 + i, gc = j * 64 + lane;
        unsigned long long w[NF + 1];
        rd.ice_words(gr >= 0 && gr < n && gc < m, (int64_t)gr * m + gc, w);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q <= NF; ++q) bits[i][j][q] = w[q];
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
            res[2 + dir] = wave_sum(sq);
            res[4 + dir] = wave_sum(sd);
            res[6 + dir] = wave_max(mx);
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

// Per-pixel verification sums: k_score_multi's reads (one PixelReader stepped over the clips), kept per pixel and summed over
// the clips instead of per clip and summed over the pixels.  One thread owns pixel p of step z and is the only writer of its 8 * S running doubles
// (maps + z * maps_step_stride, laid out (S, 8, P)): it loads the three sums of every source, adds the clips' terms to them
// one by one in clip order in double, and stores them; the class counts are integers (exact in any order) and are added to
// their running values at the end.  d = f - y is formed in fp32 as in k_score_multi and then widened; d * d of a widened fp32
// is exact in double, so contracting it into the add changes no bit.  The result is the left-to-right float64 sum over every
// clip that was ever added, however the clips were batched.  No atomics, no LDS, no cross-thread step; launches that share
// `maps` are ordered by their stream.
template <int S>
__global__ __launch_bounds__(256) void k_score_maps(ScoreArgs a, int64_t P, int B, double* __restrict__ maps,
                                                    int64_t maps_step_stride) {
    const int z = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || a.masked(p)) return;                        // a masked pixel counts in no clip: its doubles stay as they are
    PixelReader<S> rd(a, P, 0, z);
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
    for (int b = 0; b < B; ++b, rd.next_clip()) {
        const int lab = rd.label(p);
        if (!rd.node(lab)) continue;                          // with the mask test above: counted()
        const float t = rd.truth(p);
        const bool ty = t > a.thr;
        float f[S];
        rd.load(p, lab, f);
        ++n;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float d32 = f[s] - t;
            const double d = (double)d32;
            const bool tf = f[s] > a.thr;
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
// consecutive steps, per source (observed, model, optionally one dense field).  k_score_maps' reads, but along the time axis
// (a PixelReader per step; the truth is source 0 here): one thread owns pixel p of clip b, reads its label once per step and
// serves every source from it, and carries
// per source the current run length and the date in registers over the chunk's steps.  A launch with z0 == 0 initialises the
// state (date -2 under the mask, else -1; run 0, or -1 where the launch frame is already in the target state: such a pixel has
// no event, and a negative run is never advanced), a launch with z0 > 0 loads what the previous chunk stored.  A pixel without
// a valid node at any step ends as -2 for every source.  No atomics, no LDS, no cross-thread step; chunks are ordered by their
// stream.
template <int S1>
__global__ __launch_bounds__(256) void k_event_scan(ScoreArgs a, int nseg, const float* __restrict__ launch,
                                                    int64_t launch_clip_stride, int target, int k, int z0, int64_t P,
                                                    int32_t* __restrict__ dates, int32_t* __restrict__ runs) {
    const int b = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const bool g = target != 0;
    const int64_t st = ((int64_t)b * S1) * P + p;             // source s of this pixel: st + s * P
    int date[S1], run[S1];
    if (z0 == 0) {
        const int d0 = a.masked(p) ? -2 : -1;
        const int r0 = ((launch[b * launch_clip_stride + p] > a.thr) == g) ? -1 : 0;
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
    for (int z = 0; z < nseg && !dead; ++z) {
        const PixelReader<S1 - 1> rd(a, P, b, z);
        const int lab = rd.label(p);
        if (!rd.node(lab)) {                                  // the mask made the pixel dead before the first step
            dead = true;
            break;
        }
        float f[S1];
        f[0] = rd.truth(p);
        rd.load(p, lab, f + 1);
#pragma unroll
        for (int s = 0; s < S1; ++s) {
            if (run[s] < 0) continue;
            run[s] = ((f[s] > a.thr) == g) ? run[s] + 1 : 0;
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
    for (int v = 0; v < 8; ++v) acc[v] = wave_sum(acc[v]);
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

// What the rollout launchers have in common, in the order every one of them refuses: the segment arrays of 1..16 steps, the
// truth and the dense baseline fields that are present into `a`; then `own`, the reason of the entry's own first checks if
// one of them failed (else null); then the sizes, where B is at most `B_max` (a grid dimension for all but qt_score_maps).
// Returns the reason of a refusal, or null; the entry reports it under its own name (QT_ARG).
const char* score_setup(ScoreArgs& a, int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                        const int* Ns, const int32_t* const* n_devs, ScoreBase y, ScoreBase base1, ScoreBase base2,
                        const uint8_t* pix_mask, float thr, const char* own, int B, int n, int m, int B_max = 65535) {
    if (!(nseg >= 1 && nseg <= 16)) return "nseg must be 1..16";
    if (!(outs && out_strides && labels && Ns && n_devs && y.f)) return "null pointer";
    if (!(y.clip_stride >= 0 && y.step_stride >= 0 && base1.clip_stride >= 0 && base1.step_stride >= 0 &&
          base2.clip_stride >= 0 && base2.step_stride >= 0))
        return "negative stride";
    a = {};
    ScoreSeg& sg = a.sg;
    for (int z = 0; z < nseg; ++z) {
        if (!(labels[z] && Ns[z] >= 0 && (outs[z] || Ns[z] == 0) && out_strides[z] >= 1)) return "bad segment";
        sg.out[z] = outs[z]; sg.out_stride[z] = out_strides[z]; sg.labels[z] = labels[z]; sg.N[z] = Ns[z]; sg.n_dev[z] = n_devs[z];
    }
    a.y = y;
    if (base1.f) a.bs[a.nb++] = base1;
    if (base2.f) a.bs[a.nb++] = base2;
    a.pix_mask = pix_mask;
    a.thr = thr;
    if (own) return own;
    if (!(B > 0 && B <= B_max && n > 0 && m > 0)) return "bad sizes";
    return nullptr;
}

// The instantiation of a kernel template for the sources present: the model and `nb` dense fields
template <typename K>
K by_sources(int nb, K k1, K k2, K k3) {
    return nb == 0 ? k1 : nb == 1 ? k2 : k3;
}

// The first of qt_fss_rollout's own refusals, or null with the half widths in `sc`
const char* fss_scales(FssScales& sc, int nscales, const int* scales, const int32_t* partial) {
    if (!(nscales >= 1 && nscales <= 8)) return "nscales must be 1..8";
    if (!scales) return "null scales";
    sc = {};
    sc.K = nscales;
    for (int k = 0; k < nscales; ++k) {
        // the kernel's column mask and halo hold windows up to 33 wide and no wider
        if (!(scales[k] >= 1 && scales[k] <= 33 && (scales[k] & 1))) return "scales must be odd and in 1..33";
        if (!(k == 0 || scales[k] > scales[k - 1])) return "scales must be strictly increasing";
        sc.h[k] = scales[k] / 2;
    }
    return partial ? nullptr : "null partial";
}

}  // namespace

extern "C" int qt_score_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                                const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                                int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                                const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                                const uint8_t* pix_mask, float thr, int B, int n, int m, float* partial, void* stream) {
    ScoreArgs a;
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride},
                                  pix_mask, thr, partial ? nullptr : "null pointer", B, n, m);
    QT_ARG(!why, why);
    const int64_t P = (int64_t)n * m;
    // the kernel's partial rows are sized for the sources present
    hipLaunchKernelGGL(by_sources(a.nb, k_score_multi<1>, k_score_multi<2>, k_score_multi<3>), dim3(qt_cdiv(P, 1024), B, nseg),
                       dim3(256), 0, (hipStream_t)stream, a, P, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_reliability_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                                      const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                                      int64_t y_step_stride, const float* base1, int64_t base1_clip_stride,
                                      int64_t base1_step_stride, const float* base2, int64_t base2_clip_stride,
                                      int64_t base2_step_stride, const uint8_t* pix_mask, float thr, int B, int n, int m,
                                      int bins, float* partial, void* stream) {
    ScoreArgs a;
    const char* own = !(bins >= 2 && bins <= 32) ? "bins must be 2..32" : !partial ? "null partial" : nullptr;
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride},
                                  pix_mask, thr, own, B, n, m);
    QT_ARG(!why, why);
    const int64_t P = (int64_t)n * m;
    hipLaunchKernelGGL(by_sources(a.nb, k_reliability_multi<1>, k_reliability_multi<2>, k_reliability_multi<3>),
                       dim3(qt_cdiv(P, 1024), B, nseg), dim3(256), 0, (hipStream_t)stream, a, bins, P, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_extent_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                                 const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                                 int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                                 const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                                 const uint8_t* pix_mask, float thr, int B, int n, int m, const int8_t* region,
                                 const float* area, int R, float* partial, void* stream) {
    ScoreArgs a;
    // the kernel's LDS rows are sized for 32 regions
    const char* own = !(R >= 1 && R <= 32) ? "R must be 1..32" : !partial ? "null partial" : nullptr;
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride},
                                  pix_mask, thr, own, B, n, m);
    QT_ARG(!why, why);
    const int64_t P = (int64_t)n * m;
    hipLaunchKernelGGL(by_sources(a.nb, k_extent_multi<1>, k_extent_multi<2>, k_extent_multi<3>),
                       dim3(qt_cdiv(P, 1024), B, nseg), dim3(256), 0, (hipStream_t)stream, a, region, area, R, P, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_fss_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                              const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                              int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                              const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                              const uint8_t* pix_mask, float thr, int B, int n, int m, int nscales, const int* scales,
                              int32_t* partial, void* stream) {
    ScoreArgs a;
    FssScales sc;
    const char* own = fss_scales(sc, nscales, scales, partial);
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride},
                                  pix_mask, thr, own, B, n, m);
    QT_ARG(!why, why);
    const int tiles_m = qt_cdiv(m, 32);
    const int64_t ntile = (int64_t)qt_cdiv(n, 32) * tiles_m;
    QT_ARG(ntile <= 0x7fffffff, "bad sizes");
    hipLaunchKernelGGL(by_sources(a.nb, k_fss_multi<1>, k_fss_multi<2>, k_fss_multi<3>), dim3((unsigned)ntile, B, nseg),
                       dim3(256), 0, (hipStream_t)stream, a, sc, n, m, tiles_m, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_edge_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                               const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                               int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                               const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                               const uint8_t* pix_mask, float thr, int B, int n, int m, uint64_t* planes, int32_t* partial,
                               void* stream) {
    ScoreArgs a;
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride},
                                  pix_mask, thr, planes && partial ? nullptr : "null planes / partial", B, n, m);
    QT_ARG(!why, why);
    // k_edge_search holds a (step, clip)'s planes in LDS and packs a query into 16 bits; its int32 sums are proved for this size
    QT_ARG(n <= EDGE_MAX && m <= EDGE_MAX, "frame larger than 256 x 256");
    const int W = qt_cdiv(m, 64);
    const dim3 grid(qt_cdiv(n, EDGE_BAND), B, nseg);
    hipLaunchKernelGGL(by_sources(a.nb, k_edge_planes<1>, k_edge_planes<2>, k_edge_planes<3>), grid, dim3(256), 0,
                       (hipStream_t)stream, a, n, m, W, B, (unsigned long long*)planes);
    QT_LAUNCHED();
    hipLaunchKernelGGL(by_sources(a.nb, k_edge_search<1>, k_edge_search<2>, k_edge_search<3>), grid, dim3(256), 0,
                       (hipStream_t)stream, (const unsigned long long*)planes, n, W, B, partial);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_score_maps(int nseg,const float* const* outs, const int* out_strides, const int32_t* const* labels,
                             const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                             int64_t y_step_stride, const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride,
                             const float* base2, int64_t base2_clip_stride, int64_t base2_step_stride,
                             const uint8_t* pix_mask, float thr, int B, int n, int m, double* maps, int64_t maps_step_stride,
                             void* stream) {
    ScoreArgs a;
    // the clips are a loop in the kernel and no grid dimension: B has no upper bound
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base1, base1_clip_stride, base1_step_stride}, {base2, base2_clip_stride, base2_step_stride},
                                  pix_mask, thr, maps ? nullptr : "null pointer", B, n, m, 0x7fffffff);
    QT_ARG(!why, why);
    const int64_t P = (int64_t)n * m;
    // a step's (S, 8, P) block must fit its stride, or step z would write into step z + 1
    QT_ARG(maps_step_stride >= (int64_t)(1 + a.nb) * 8 * P, "maps_step_stride is smaller than S*8*n*m");
    hipLaunchKernelGGL(by_sources(a.nb, k_score_maps<1>, k_score_maps<2>, k_score_maps<3>), dim3(qt_cdiv(P, 256), nseg),
                       dim3(256), 0, (hipStream_t)stream, a, P, B, maps, maps_step_stride);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_event_scan(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                             const int* Ns, const int32_t* const* n_devs, const float* y, int64_t y_clip_stride,
                             int64_t y_step_stride, const float* base, int64_t base_clip_stride, int64_t base_step_stride,
                             const uint8_t* pix_mask, float thr, int B, int n, int m, const float* launch,
                             int64_t launch_clip_stride, int target, int k, int z0, int32_t* dates, int32_t* runs,
                             void* stream) {
    ScoreArgs a;
    const char* own = !launch ? "null pointer" : !(dates && runs) ? "null dates / runs" : nullptr;
    const char* why = score_setup(a, nseg, outs, out_strides, labels, Ns, n_devs, {y, y_clip_stride, y_step_stride},
                                  {base, base_clip_stride, base_step_stride}, {}, pix_mask, thr, own, B, n, m);
    QT_ARG(!why, why);
    QT_ARG(launch_clip_stride >= 0, "negative stride");
    QT_ARG(target == 0 || target == 1, "target must be 0 (no ice: break-up) or 1 (ice: freeze-up)");
    QT_ARG(k >= 1, "k (persist) must be >= 1");
    QT_ARG(z0 >= 0, "z0 must be >= 0");
    const int64_t P = (int64_t)n * m;
    hipLaunchKernelGGL(a.nb ? k_event_scan<3> : k_event_scan<2>, dim3(qt_cdiv(P, 256), B), dim3(256), 0, (hipStream_t)stream, a,
                       nseg, launch, launch_clip_stride, target, k, z0, P, dates, runs);
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
