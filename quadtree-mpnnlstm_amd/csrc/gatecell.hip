// The gate-cell launches of the recurrent cells (hidden 8 / 16; operands and argument block: qt_gemm.h, cell arithmetic: qt_cell.h):
//   k_gate_cell_p    -- forward: the persistent gate GEMM Y = [T_0 .. T_{K-1} | S] W with the LSTM cell as each wave's epilogue
//   k_dgrad_cell     -- backward: the cell backward feeding the data gradient gG W^T from LDS
//   k_cell_bwd_fused -- backward, opt-in: cell backward, data gradient and weight gradient in one persistent launch
// qt_dense_lstm's other shapes (hidden 32, long reductions) take k_gemm_fwd's fused epilogue in gemm.hip.
// What these kernels share with lstm.hip and gemm.hip stands once: in qt_cell.h the cell arithmetic, cell_params / cell_bwd_params,
// the backward's operand read (cell_bwd_load), ld_gates / st_gates and block_param_reduce; in qt_gemm.h the quad table
// (build_quad_table), the MFMA step of a k-quad (mfma_quad), the accumulator row map (acc_row) and store_split.  Where a kernel
// still spells one of these out, the comment at the site says what the helper changed in its generated code (HISTORY.md, AL).
#include "qt_cell.h"
#include "qt_gemm.h"

namespace {

// ---- persistent gate GEMM + LSTM cell (hidden 8 / 16): one 512-thread workgroup per CU, W staged ONCE, no workgroup barrier
// after that.  The unit of work is a WAVE's 32 node rows x all 4h gate columns: the wave streams its A quads global -> VGPR
// through a 4-deep ring that already holds the next unit's first quads when the current unit's epilogue starts, runs the
// MFMA chain, parks the accumulators in its OWN staging rows in LDS and computes the cell for those 32 nodes itself (h / 4
// lanes per node, as k_gemm_fwd's fused epilogue: same arithmetic in the same order, bit-identical results).  Two waves
// share a SIMD, so one wave's epilogue (VALU, LDS, stores) runs beside the other's MFMA chain.  Against the one-tile
// workgroups of k_gemm_fwd<2, 128, 4> this removes the per-tile W staging (4 us of 21 at the bench shape), the four
// workgroup barriers per tile, and the serial memory -> MFMA -> store phases of a tile.
// Work split: workgroup b owns the contiguous units [U b / G, U (b + 1) / G) of the U = ceil(rows / 32) units (valid rows
// read on the device), its wave w takes every 8th of them.
constexpr int GATE_P_MAXK = 256, GATE_P_MAXPITCH = GATE_P_MAXK + 8;
template <int NT, int LPN, int R>
__global__ __launch_bounds__(512, 2) void k_gate_cell_p(GemmArgs g, int pitch) {
    using namespace qtcell;
    constexpr int BNT = 32 * NT, h = 4 * LPN, CP = 5 * h, NPW = 64 / LPN, NPASS = 32 / NPW;
    static_assert(4 * h == BNT, "the gate columns fill the MFMA tiles exactly");
    // static LDS (a single workgroup may declare up to 160 KiB on gfx950; dynamic LDS beyond 64 KiB was refused at launch)
    __shared__ __attribute__((aligned(16))) float Bt[BNT * GATE_P_MAXPITCH];   // W^T: [BNT][pitch], pitch / 4 odd -> conflict-free ds_read_b128
    __shared__ __attribute__((aligned(16))) float Cst[8 * 32 * CP];
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    float* Cs = Cst + wave * (32 * CP);                 // this wave's staging rows
    const int rows = qt_rows(g.n_dev, g.M);
    const int nunits = (rows + 31) >> 5;
    const int u0 = (int)((int64_t)nunits * blockIdx.x / gridDim.x), u1 = (int)((int64_t)nunits * (blockIdx.x + 1) / gridDim.x);
    if (u0 >= u1) return;
    const int nquad = g.K >> 2;
    build_quad_table(g.A, qptr, qstr, nquad);
    if (g.BT) {
        for (int e = t; e < BNT * nquad; e += 512) {
            const int c = e / nquad, kq = e - c * nquad;
            *reinterpret_cast<float4*>(&Bt[c * pitch + 4 * kq]) = *reinterpret_cast<const float4*>(g.BT + (int64_t)c * g.K + 4 * kq);
        }
    } else {
        for (int e = t; e < g.K * (BNT / 4); e += 512) {
            const int kb = e / (BNT / 4), jq = (e % (BNT / 4)) * 4;
            const float4 w = *reinterpret_cast<const float4*>(g.B + (int64_t)kb * BNT + jq);
            Bt[(jq + 0) * pitch + kb] = w.x;
            Bt[(jq + 1) * pitch + kb] = w.y;
            Bt[(jq + 2) * pitch + kb] = w.z;
            Bt[(jq + 3) * pitch + kb] = w.w;
        }
    }
    if (g.K & 4)                                          // an odd quad count: the last k-group's upper half reads zeros
        for (int c = t; c < BNT; c += 512) *reinterpret_cast<float4*>(&Bt[c * pitch + g.K]) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();                                      // the only workgroup barrier
    int unit = u0 + wave;
    if (unit >= u1) return;
    const int nj = (g.K + 7) >> 3;
    // Every A load is UNCONDITIONAL (row and quad clamped to valid ones): a load inside a branch makes hipcc's s_waitcnt
    // bookkeeping fall back to draining the whole queue at the next use, which serialised the stream (41 us per launch at
    // the bench shape, whatever the ring depth).  A row past the valid ones re-reads the last valid row: an accumulator
    // row depends on its own A row only and the epilogue stores no such row, so its values need no zeroing.  Only a quad
    // past the last one is zeroed (an odd quad count: the upper half of the last k-group; with R > 0 that can only be
    // ring slot R - 1, as nj == R means nquad >= 2 R - 1).  The row is a 32-bit int (rows is one), so row x stride is one
    // 32 x 32 -> 64-bit multiply-add; with R > 0 the table entries of slot j are the same for every unit and stay in registers.
    const int last_row = rows - 1;
    const float* qp[R > 0 ? R : 1];
    int qs[R > 0 ? R : 1];
    if constexpr (R > 0) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int q = 2 * j + half, qc = q < nquad ? q : 0;
            qp[j] = qptr[qc];
            qs[j] = qstr[qc];
        }
    }
    auto ldq = [&](int row, int j) {          // row: already clamped to the valid ones
        const int q = 2 * j + half;
        if constexpr (R > 0) {
            const float4 r = gload4(qp[j] + (int64_t)row * qs[j]);
            if (j < R - 1) return r;
            const bool use = q < nquad;
            return make_float4(use ? r.x : 0.f, use ? r.y : 0.f, use ? r.z : 0.f, use ? r.w : 0.f);
        } else {
            const bool use = q < nquad;
            const int qc = use ? q : 0;
            const float4 r = gload4(qptr[qc] + (int64_t)row * qstr[qc]);
            return make_float4(use ? r.x : 0.f, use ? r.y : 0.f, use ? r.z : 0.f, use ? r.w : 0.f);
        }
    };
    int my_row = min(unit * 32 + l32, last_row);
    // The A operand is streamed once and shared with no other wave: it goes global -> VGPR, and what bounds the stream is the
    // bytes a CU keeps in flight (8 waves x 4 quads of 1 KiB = 32 KiB ran at 2.5 TB/s).  R > 0: the ring holds a WHOLE unit
    // (nj <= R steps, the j loop fully unrolled so that ring[j] is a fixed register): step j consumes ring[j] and at once
    // requests the next unit's quad j into it, so a wave always has ~nj KiB in flight, across the epilogue too.
    // R == 0 (any nj): the 4-deep rotating ring of k_gemm_fwd.
    float4 ring[R > 0 ? R : 4];
#pragma unroll
    for (int j = 0; j < (R > 0 ? R : 4); ++j) ring[j] = ldq(my_row, j);
    const int nl = lane / LPN, j0 = (lane - nl * LPN) * 4;
    const CellParams cpar = cell_params(g.wc, g.bias, g.ln, h, j0);      // in registers for the whole launch
    while (true) {
        // this unit's previous cell states (one node per epilogue pass and lane group): requested before the MFMA chain
        float4 cpre[NPASS];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int64_t node = (int64_t)unit * 32 + ps * NPW + nl;
            cpre[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (node < rows && g.Cprev) cpre[ps] = *reinterpret_cast<const float4*>(g.Cprev + node * g.ld_c + j0);
        }
        const int nxt = unit + 8;
        const bool has_next = nxt < u1;
        const int nrow = has_next ? min(nxt * 32 + l32, last_row) : last_row;       // (no next unit: a valid address, unused values)
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
        auto step = [&](const float4& a, int j) {
            float4 bq[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                bq[nt] = *reinterpret_cast<const float4*>(&Bt[(nt * 32 + l32) * pitch + 8 * j + 4 * half]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mfma_quad(acc[nt], a, bq[nt]);
        };
        if constexpr (R > 0) {
#pragma unroll
            for (int j = 0; j < R; ++j) {     // nj == R (the host picks the instance): straight-line code, no branch
                const float4 a = ring[j];
                ring[j] = ldq(nrow, j);
                step(a, j);
            }
        } else {
            for (int j = 0; j < nj; ++j) {
                const float4 a = ring[0];
                ring[0] = ring[1]; ring[1] = ring[2]; ring[2] = ring[3];
                ring[3] = ldq(my_row, j + 4);
                step(a, j);
            }
            // the next unit's first quads fly during this unit's epilogue
#pragma unroll
            for (int j = 0; j < 4; ++j) ring[j] = ldq(nrow, j);
        }
        // epilogue: accumulator columns -> this wave's staging rows -> h / 4 lanes per node
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) Cs[acc_row(r, half) * CP + u * 32 + l32] = acc[u][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int row = ps * NPW + nl;
            const int64_t node = (int64_t)unit * 32 + row;
            F4 gi, gf, gc, go;
            ld_gates(Cs + row * CP + j0, h, &gi, &gf, &gc, &go);
            const F4 cp = {{cpre[ps].x, cpre[ps].y, cpre[ps].z, cpre[ps].w}};
            const CellOut r = cell_forward<LPN>(gi, gf, gc, go, cp, cpar);
            if (node < rows) {          // (store_cell's text: through the helper the hidden-16 instances order their address arithmetic differently)
                if (g.O) st4(g.O + node * h + j0, r.Og);
                st4(g.Hn + node * h + j0, r.hn);
                st4(g.Cn + node * h + j0, r.cn);
                st_gates(g.gates + node * 4 * h + j0, h, r.I, r.F, r.T, r.Og);
            }
        }
        if (!has_next) break;
        unit = nxt; my_row = nrow;
    }
}

// ---- cell backward fused into the data-gradient GEMM of the gate weights (hidden 8 / 16).
// gG = d loss / d gate pre-activations comes out of the cell backward (k_lstm_bwd's arithmetic, qt_cell.h) and is at once
// the left operand of  gT = gG W^T  (K = 4h reduction, all output planes in this workgroup's 32 NT columns).  Here a
// workgroup computes the gG rows of its 128 nodes into LDS (and to global memory: the deferred weight gradient reads them),
// then feeds the MFMA loop from LDS: the (N, 4h) matrix is not read back from memory and one launch per use is gone.
// Same operand order as k_gemm_fwd on the stored gG: bit-identical planes.
struct DgradCellArgs {
    const float *gO, *gHn, *gCn, *gates, *Cprev, *wc, *ln;
    int ld_go, ld_gh, ld_gc, ld_c, h;
    float *gG, *gCprev, *part;
    int accumulate;
    const float* BT;        // (NB, 4h): rows k*C + c of the forward weight (= the transposed right operand)
    const __bf16 *BThi, *BTlo;   // optional: the same rows split into two bf16 terms (qt_split_bf16): the product runs on bf16 MFMA
    int M, NB, Kb, Cb, Cbb;
    float *out, *outb;
    const int32_t* n_dev;
    int out_sm;             // output planes 1 .. Kb-1 slice-major (plane_piece)
    // Two gradient sums that autograd would otherwise make with separate elementwise launches (a tensor with two consumers):
    const float* gHn2;      // optional second gradient of H' (the state goes to the next time step AND to the next layer): added on load
    int ld_gh2;
    const float* add0;      // optional (N, Cb): added to output plane 0 of part a (the decoder input is also the head's residual
                            // operand: that gradient rides into the Clenshaw recurrence as part of A_0)
};

// The right operand (the weight rows, <= 32 KB, L1 / L2 resident) is read straight from global memory by the lanes that need
// it and is not staged in LDS: the workgroup's LDS is 38 KB where the staged form took 64 KB, so more than two workgroups fit
// a CU -- more workgroups whose load / arithmetic / MFMA / store phases overlap (the staged form's numbers: HISTORY.md, AL).
static constexpr int QT_DGRAD_OCC = 4;      // 128 VGPRs (hidden 16: 5 spilled, 20 bytes of scratch; 9 before gG left from LDS): FOUR workgroups per CU = all 940 tiles of the bench shape resident at once
                          // (3: 138-155 VGPRs, 768 resident + a second round; 8.41 -> 8.34 ms per frozen step)
template <int NT, int LPN>
__global__ __launch_bounds__(256, QT_DGRAD_OCC) void k_dgrad_cell(DgradCellArgs g) {
    using namespace qtcell;
    constexpr int K = 16 * LPN, PITCH = K + 4, RP = 256 / LPN;
    __shared__ __attribute__((aligned(16))) float As[128 * (PITCH > 68 ? PITCH : 68)];       // (>= 128 x 68: the epilogue's staging tile)
    __shared__ float sm[4 * LPN * 11 * 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const int64_t rows = qt_rows(g.n_dev, g.M);
    constexpr int h = 4 * LPN;     // (== g.h: the host picks the instance by it)
    // gG rows leave whole, from the LDS tile behind the first barrier (below), at hidden 16 only: at hidden 8 the cell phase's
    // stores already take 32 bytes of a 128-byte row per lane pair, and the launch was 0.7 - 1.2 us SLOWER with the row stores
    // (27.7 -> 28.4 - 28.9 us at 120 k rows, profiles/dgrad_cell_rows.txt), so those instances keep the parent's code.
    constexpr bool GG_ROWS = LPN == 4;
    if (i0 >= rows) return;        // past the valid rows: nothing to add to the partials (the slab rows start at zero)
    // cell backward of this workgroup's rows (rows past the valid count contribute zeros)
    {
        const int j0 = (t % LPN) * 4;
        const CellBwdParams P = cell_bwd_params(g.wc, g.ln, h, j0);
        float acc[11][4];
#pragma unroll
        for (int a = 0; a < 11; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[a][k] = 0.0f;
#pragma unroll
        for (int r0 = 0; r0 < BM; r0 += RP) {
            const int r = r0 + t / LPN;
            const int64_t node = i0 + r;
            const bool ok = node < rows;
            const CellBwdIn x = cell_bwd_load(ok, node, h, j0, g.gates, g.Cprev, g.ld_c, g.gHn, g.ld_gh, g.gCn, g.ld_gc, g.gO,
                                              g.ld_go, g.gHn2, g.ld_gh2);
            const CellBwdOut o = cell_backward<LPN>(x, P, acc);
            st_gates(As + r * PITCH + j0, h, o.ggi, o.ggf, o.ggc, o.ggo);
            if (ok) {
                if constexpr (!GG_ROWS) st_gates(g.gG + node * 4 * h + j0, h, o.ggi, o.ggf, o.ggc, o.ggo);
                if (g.gCprev) st4(g.gCprev + node * h + j0, o.gcp);
            }
        }
        block_param_reduce<LPN, 11>(acc, h, sm, g.part + (int64_t)blockIdx.x * 11 * h, g.accumulate);
    }
    qt_lds_barrier();                                 // As complete
    // Hidden 16: gG (the deferred weight gradient reads it) leaves from the finished tile, not from the cell phase.  There a lane
    // owns the four h-apart quarters of its node's row, so a store instruction of a wave touched 16 rows and took 64 bytes of each,
    // half a 128-byte line.  The tile's rows are one contiguous run of BM x 4h floats in gG: thread t takes the float4 pieces
    // t, t + 256, .. of the run -- a wave 1 KB, four whole rows, per instruction -- and the stores drain under the MFMA loop.  The
    // values are the ones the cell phase wrote to As: the same bits.  All pieces are read before the first store (a read inside the
    // store's branch waited for LDS eight times in a row).  LDS side (ds_read_b128: four 16-lane groups, bank = word mod 64): the
    // pitch of 68 floats shifts consecutive rows by one 16-byte slot, so two of the groups (lanes 4-11 with 16-19: pieces 4 and 3 of neighbouring rows) meet one slot
    // twice: 6 LDS cycles where a conflict-free map takes 4, on 8 instructions a thread.  The pitch is the MFMA operand read's and stays.
    if constexpr (GG_ROWS) {
        constexpr int NP = BM * (K / 4) / 256;
        const int nvalid = (int)min((int64_t)BM, rows - i0) * (K / 4);     // the float4 pieces of the valid rows: no row at or past the count is written
        float* gq = g.gG + i0 * K;
        float4 v[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int e = t + 256 * u;
            v[u] = *reinterpret_cast<const float4*>(&As[(e / (K / 4)) * PITCH + (e % (K / 4)) * 4]);
        }
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int e = t + 256 * u;
            if (e < nvalid) *reinterpret_cast<float4*>(gq + 4 * e) = v[u];
        }
    }
    f32x16 acc2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[nt][r] = 0.0f;
    if (g.BThi) {
        // OPT-IN split-bf16 product (ops.DGRAD_SPLIT_BF16; backward only; the default is the exact fp32 branch below): gG = hi + lo, W = Whi + Wlo (two bf16 terms each, the
        // weight split once per pass by qt_split_bf16), gG W^T ~ hi Whi + hi Wlo + lo Whi -- relative error ~2^-16 per
        // product -- on v_mfma_f32_32x32x16_bf16: 3 MFMAs of 32 cycles per 16 k instead of 8 fp32 MFMAs of 64 cycles (the
        // fp32 MFMA issues on the vector pipe: its 10.7 us per launch at the bench shape added to the cell arithmetic).
        // Lane (r = l & 31, hh = l >> 5) holds A[row r][k = 16 s + 8 hh + j] and B[k = 16 s + 8 hh + j][column r], j = 0 .. 7.
#pragma unroll
        for (int s_ = 0; s_ < K / 16; ++s_) {
            const float* ap = &As[(wave * 32 + l32) * PITCH + 16 * s_ + 8 * half];
            const float4 a0 = *reinterpret_cast<const float4*>(ap), a1 = *reinterpret_cast<const float4*>(ap + 4);
            const float af[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            bf16x8 ahi, alo;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const __bf16 hq = (__bf16)af[q];
                ahi[q] = hq;
                alo[q] = (__bf16)(af[q] - (float)hq);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c = nt * 32 + l32;                  // (columns past NB: clamped load, zeroed value)
                const int64_t off = (int64_t)(c < g.NB ? c : 0) * K + 16 * s_ + 8 * half;
                bf16x8 bhi = *(const __attribute__((address_space(1))) bf16x8*)(g.BThi + off);
                bf16x8 blo = *(const __attribute__((address_space(1))) bf16x8*)(g.BTlo + off);
                if (c >= g.NB) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) { bhi[q] = (__bf16)0.0f; blo[q] = (__bf16)0.0f; }
                }
                acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, acc2[nt], 0, 0, 0);
                acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, acc2[nt], 0, 0, 0);
                acc2[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, acc2[nt], 0, 0, 0);
            }
        }
    } else {
#pragma unroll
    for (int j = 0; j < K / 8; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(&As[(wave * 32 + l32) * PITCH + 8 * j + 4 * half]);
        float4 bq[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            // (columns past NB: a clamped load.  An accumulator column depends on its own column of the operand only and
            // the epilogue stores no column past NB, so the value needs no zeroing: 4 NT selects per k-group saved)
            const int c = nt * 32 + l32;
            bq[nt] = gload4(g.BT + (int64_t)(c < g.NB ? c : 0) * K + 8 * j + 4 * half);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) mfma_quad(acc2[nt], a, bq[nt]);
    }
    }
    // epilogue as in k_gemm_fwd: the tile goes through LDS (As is free now) so that rows leave as float4 pieces.  The staging
    // tile has a pitch of 68 floats (As holds 128 x 68): with slice-major output planes a wave stores 64 consecutive ROWS of one
    // 4-channel piece -- 1 KB contiguous in that slice's array -- and reads them from LDS at a 272-byte stride, which the 64
    // banks take without conflicts (a 256-byte stride would hit one bank group 16 times).
    float* Cs = As;
    constexpr int CP = 68;
#pragma unroll
    for (int h2 = 0; h2 < (NT + 1) / 2; ++h2) {
        qt_lds_barrier();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int nt = 2 * h2 + u;
            if (nt < NT) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Cs[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * CP + u * 32 + l32] = acc2[nt][r];   // (acc_row's text: the helper's sum associates differently and two vector instructions change place)
            }
        }
        qt_lds_barrier();
#pragma unroll
        for (int u = 0; u < BM * 16 / 256; ++u) {
            const int e = t + 256 * u;
            // row-major planes: 16 consecutive lanes take the 16 pieces of one row (64-byte runs per plane); slice-major planes:
            // 128 consecutive threads take the 128 rows of one piece
            const int row = g.out_sm ? (e & 127) : (e >> 4), c4 = (g.out_sm ? (e >> 7) : (e & 15)) * 4;
            const int64_t i = i0 + row;
            const int j = h2 * 64 + c4;
            if (i >= rows || j >= g.NB) continue;
            const float4 v = *reinterpret_cast<const float4*>(&Cs[row * CP + c4]);
            store_split(g.out, g.outb, g.Cb, g.Cbb, g.M, g.out_sm, j, i, v, g.Cb, g.add0);
        }
    }
}

// ---- the whole backward pass of one gate-cell use in ONE persistent launch (hidden 8 / 16): cell backward, the data gradient
// gT = gG W^T AND the weight gradient gW = [T_0 .. T_{K-1} | S]^T gG.  The gate gradients gG (N, 4h) never exist in memory:
// a workgroup (one per CU, 512 threads) walks its share of the 128-row tiles, computes a tile's gG rows into LDS, feeds both
// MFMA products from there and keeps its partial gW (<= 128 x 64) in accumulator registers across all its tiles -- one slab
// per workgroup at the end, summed over the workgroups (and over the uses of the weight in the pass) by qt_colsum, in a
// fixed order.  Against qt_lstm_bwd_dgrad + the deferred qt_wgrad_group this drops the gG round trip (31 MB written and
// read back per use at the bench shape) and the separate weight-gradient launches, and the weight gradient's left operand
// is read while it is still warm from nothing -- it is read once either way -- but beside the cell's own traffic.
//   per tile:  TZ tile (128 x K) global -> LDS, row major (8 float4 in flight per thread)
//              cell backward of the 128 nodes (h / 4 lanes per node, k_lstm_bwd's arithmetic) -> gG tile in LDS, gCprev
//              barrier
//              wave w: weight-gradient tile (i block w & 3, j block w >> 2): 64 x mfma_32x32x2 over the 128 rows
//                      data-gradient tiles of row group w & 3 (column tiles split between waves 0-3 and 4-7)
//              barrier; data-gradient tiles -> LDS (over the TZ tile) -> row-contiguous float4 stores; barrier
struct CellBwdFusedArgs {
    DgradCellArgs d;          // cell operands, gCprev, part, BT = Wrows, NB, Kb, Cb, Cbb, out, outb, M (capacity), n_dev; gG unused
    PlaneSrc A;               // [T_0 .. T_{K-1} | S] of the forward pass
    int Kt;                   // rows of W: K * C + padded bias rows (<= 128)
    float* slab;              // (gridDim.x, Kt, 4h): this launch ADDS its partial weight gradients (zeroed by the caller)
};

// The opt-in kernel keeps its own copies of the column sum (block_param_reduce of qt_cell.h with the wave count as a parameter,
// the butterfly through __shfl_xor, a full barrier) and of the quad table (build_quad_table of qt_gemm.h).  Its 64-row instances
// sit at 254 - 256 VGPRs: with either shared piece, or with the shared operand read and stores, they spill 36 - 44 bytes more,
// and the launch took 63.1 us against 60.2 at the bench shape (HISTORY.md, AL).  Same bits either way.
template <int LPN, int NW, int NACC>
__device__ __forceinline__ void block_param_reduce_n(float (&acc)[NACC][4], int h, float* sm, float* part_row, int accumulate) {
    using namespace qtcell;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v = acc[a][k];
#pragma unroll
            for (int d = LPN; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
            acc[a][k] = v;
        }
    if (lane < LPN) {
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) sm[(wave * LPN + lane) * NACC * 4 + a * 4 + k] = acc[a][k];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NACC * h; idx += 64 * NW) {
        const int a = idx / h, j = idx % h;
        const int li = j >> 2, k = j & 3;
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += sm[(w * LPN + li) * NACC * 4 + a * 4 + k];
        part_row[idx] = accumulate ? part_row[idx] + s : s;
    }
}

// TR = rows per tile (threads = 4 TR): 64 -> two 256-thread workgroups per CU whose phases (loads + cell arithmetic / MFMA /
// stores) drift apart and overlap; 128 -> one 512-thread workgroup per CU (every phase of the CU in lockstep: 71 us per launch
// at the bench shape against 68 us for the separate launches it replaces).
constexpr int fused_tile_rows(int nt) { return nt <= 3 ? 64 : 128; }      // nt: 32-column tiles of the data gradient
template <int NT, int LPN, int TR = fused_tile_rows(NT)>
__global__ __launch_bounds__(4 * TR, 2) void k_cell_bwd_fused(CellBwdFusedArgs f) {
    using namespace qtcell;
    const DgradCellArgs& g = f.d;
    constexpr int h = 4 * LPN, G4 = 4 * h, GP = G4 + 4, TP = 128, NJB = G4 / 32, NTA = (NT + 1) / 2;
    constexpr int NTHR = 4 * TR, NWAVE = NTHR / 64, NRG = TR / 32;            // waves = 2 NRG: (row group, column-tile half)
    constexpr int NWT = (4 * NJB + NWAVE - 1) / NWAVE;                        // weight-gradient tiles per wave
    constexpr int RSTEP = NTHR / 32, NU = TR / RSTEP;                         // TZ quads per thread (8)
    __shared__ __attribute__((aligned(16))) float TZt[TR * TP];       // TZ tile [row][k]; later the data-gradient staging tile
    __shared__ __attribute__((aligned(16))) float Gt[TR * GP];        // gG tile [row][4h]
    __shared__ __attribute__((aligned(16))) float Bt[32 * NT * GP];   // Wrows [column][4h]
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    __shared__ float sm[NWAVE * LPN * 11 * 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    const int rows = qt_rows(g.n_dev, g.M);
    const int ntiles = (rows + TR - 1) / TR;
    const int t0 = (int)((int64_t)ntiles * blockIdx.x / gridDim.x), t1 = (int)((int64_t)ntiles * (blockIdx.x + 1) / gridDim.x);
    float* part_row = g.part + (int64_t)blockIdx.x * 11 * h;
    if (t0 >= t1) {                 // no tile for this workgroup: its slab rows keep what they hold (the launch only adds)
        if (!g.accumulate)
            for (int idx = t; idx < 11 * h; idx += NTHR) part_row[idx] = 0.0f;
        return;
    }
    const int nquad = f.Kt >> 2;
    for (int Q = t; Q < nquad; Q += NTHR) {              // (build_quad_table's text: see the note above the kernel)
        const PlaneSrc& A = f.A;
        const int ct = A.Ca + A.Cab;
        const int k = 4 * Q, kc = A.Ka * ct;
        if (k < kc) {
            const int pl = k / ct, c = k - pl * ct;
            if (c < A.Ca) {
                if (pl > 0 && A.sm) {
                    qptr[Q] = A.a_rest + ((int64_t)(pl - 1) * (A.Ca / 4) + c / 4) * A.N * 4;
                    qstr[Q] = 4;
                } else {
                    qptr[Q] = (pl == 0 ? A.a0 : A.a_rest + (int64_t)(pl - 1) * A.N * A.Ca) + c;
                    qstr[Q] = pl == 0 ? A.lda0 : A.Ca;
                }
            } else {
                if (pl > 0 && A.sm) {
                    qptr[Q] = A.a_restb + ((int64_t)(pl - 1) * (A.Cab / 4) + (c - A.Ca) / 4) * A.N * 4;
                    qstr[Q] = 4;
                } else {
                    qptr[Q] = (pl == 0 ? A.a0b : A.a_restb + (int64_t)(pl - 1) * A.N * A.Cab) + (c - A.Ca);
                    qstr[Q] = pl == 0 ? A.lda0b : A.Cab;
                }
            }
        } else {
            qptr[Q] = A.S + (k - kc);
            qstr[Q] = A.Ks;
        }
    }
    for (int e = t; e < 32 * NT * (G4 / 4); e += NTHR) {
        const int c = e / (G4 / 4), kq = e - c * (G4 / 4);
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < g.NB) w = *reinterpret_cast<const float4*>(g.BT + (int64_t)c * G4 + 4 * kq);
        *reinterpret_cast<float4*>(&Bt[c * GP + 4 * kq]) = w;
    }
    const int j0 = (t % LPN) * 4;
    float pacc[11][4];
#pragma unroll
    for (int a = 0; a < 11; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) pacc[a][k] = 0.0f;
    f32x16 accw[NWT];               // this wave's tiles of the partial weight gradient
#pragma unroll
    for (int v = 0; v < NWT; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) accw[v][r] = 0.0f;
    const int rg = wave % NRG, own = wave / NRG;
    __syncthreads();                // quad table, Bt

    const int Qq = t & 31, rb = t >> 5;
    const bool qok = Qq < nquad;
    const float* qp = qptr[qok ? Qq : 0];
    const int qs = qstr[qok ? Qq : 0];
    const int crow = t / LPN;
    float4 tz[NU];
    auto load_tz = [&](int tile) {
        const int64_t i0 = (int64_t)tile * TR;
        // thread (Q = t & 31, row = (t >> 5) + RSTEP u); quads beyond K and rows beyond the valid count are zeros (the capacity
        // rows of a static-mode operand hold garbage); the loads themselves are unconditional (clamped addresses)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int64_t row = i0 + rb + RSTEP * u;
            const bool ok = qok && row < rows;
            const float4 v = gload4(qp + (row < rows ? row : (int64_t)rows - 1) * qs);
            tz[u] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
        }
    };
    load_tz(t0);
    for (int tile = t0; tile < t1; ++tile) {
        const int64_t i0 = (int64_t)tile * TR;
        // (1) cell backward of the TR nodes (LPN lanes each) -> gG tile; the TZ quads (requested one tile ahead) -> LDS while
        // the cell operands are on their way
        {
            const int64_t node = i0 + crow;
            const bool act = t < TR * LPN, ok = act && node < rows;
            const F4 z = {{0, 0, 0, 0}};
            F4 I = z, F = z, T = z, Og = z, cp = z, gyh = z, gyc = z, go_in = z;
            if (ok) {
                const float* gs = g.gates + node * 4 * h + j0;
                I = ld4(gs); F = ld4(gs + h); T = ld4(gs + 2 * h); Og = ld4(gs + 3 * h);
                if (g.Cprev) cp = ld4(g.Cprev + node * g.ld_c + j0);
                if (g.gHn) gyh = ld4(g.gHn + node * g.ld_gh + j0);
                if (g.gCn) gyc = ld4(g.gCn + node * g.ld_gc + j0);
                if (g.gO) go_in = ld4(g.gO + node * g.ld_go + j0);
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) *reinterpret_cast<float4*>(&TZt[(rb + RSTEP * u) * TP + 4 * Qq]) = tz[u];
            if (act) {
                const F4 wci = ld4(g.wc + j0), wcf = ld4(g.wc + h + j0), wco = ld4(g.wc + 2 * h + j0);
                F4 gam_h = {{1, 1, 1, 1}}, gam_c = {{1, 1, 1, 1}};
                if (g.ln) {
                    gam_h = ld4(g.ln + j0);
                    gam_c = ld4(g.ln + 2 * h + j0);
                }
                const CellBwdOut o = cell_backward<LPN>(CellBwdIn{I, F, T, Og, cp, gyh, gyc, go_in}, CellBwdParams{wci, wcf, wco, gam_h, gam_c, g.ln != nullptr}, pacc);
                float* as = Gt + crow * GP + j0;
                st4(as, o.ggi); st4(as + h, o.ggf); st4(as + 2 * h, o.ggc); st4(as + 3 * h, o.ggo);
                if (ok && g.gCprev) st4(g.gCprev + node * h + j0, o.gcp);
            }
        }
        __syncthreads();            // TZt, Gt complete
        if (tile + 1 < t1) load_tz(tile + 1);          // in flight during the MFMA phase
        // (2) weight gradient: rows 2 s + half of the tile are the two k slots of step s; the operands of the next 4 steps
        // are read from LDS before the current 4 MFMAs issue
#pragma unroll
        for (int v = 0; v < NWT; ++v) {
            const int tau = wave + NWAVE * v, ib = tau & 3, jb = tau >> 2;
            if (jb < NJB) {
                const float* ap = TZt + half * TP + 32 * ib + l32;
                const float* bp = Gt + half * GP + 32 * jb + l32;
                float av[4], bv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { av[q] = ap[2 * q * TP]; bv[q] = bp[2 * q * GP]; }
#pragma unroll 1
                for (int s0 = 0; s0 < TR / 2; s0 += 4) {
                    float an[4], bn[4];
                    const int sn = s0 + 4 < TR / 2 ? s0 + 4 : s0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) { an[q] = ap[2 * (sn + q) * TP]; bn[q] = bp[2 * (sn + q) * GP]; }
#pragma unroll
                    for (int q = 0; q < 4; ++q) accw[v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], accw[v], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) { av[q] = an[q]; bv[q] = bn[q]; }
                }
            }
        }
        // (3) data gradient of row group rg, one column tile per pass: the first half of the waves takes tile 2 ps, the second
        // half tile 2 ps + 1; the tile goes through LDS (over the TZ tile, once every wave is done with it) so that rows leave
        // as float4 pieces
        float* Cs = TZt;
#pragma unroll
        for (int ps = 0; ps < NTA; ++ps) {
            const int nt = 2 * ps + own;
            f32x16 acc2;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[r] = 0.0f;
            if (nt < NT) {
#pragma unroll
                for (int j = 0; j < G4 / 8; ++j) {
                    const float4 a = *reinterpret_cast<const float4*>(&Gt[(rg * 32 + l32) * GP + 8 * j + 4 * half]);
                    const float4 b = *reinterpret_cast<const float4*>(&Bt[(nt * 32 + l32) * GP + 8 * j + 4 * half]);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc2, 0, 0, 0);
                }
            }
            __syncthreads();        // pass 0: every wave is done with the TZ tile; later passes: the stores have read the staging tile
            if (nt < NT) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Cs[(rg * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 64 + own * 32 + l32] = acc2[r];
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = t + NTHR * u;
                const int row = e >> 4, c4 = (e & 15) * 4;
                const int64_t i = i0 + row;
                const int j = ps * 64 + c4;
                if (i < rows && j < g.NB) {
                    const float4 v = *reinterpret_cast<const float4*>(&Cs[row * 64 + c4]);
                    const int ct = g.Cb + g.Cbb;
                    const int pl = j / ct, ch = j - pl * ct;
                    if (ch < g.Cb)
                        *reinterpret_cast<float4*>(plane_piece(g.out, pl, i, ch, g.Cb, g.M, g.out_sm, g.Cb)) = v;
                    else
                        *reinterpret_cast<float4*>(plane_piece(g.outb, pl, i, ch - g.Cb, g.Cbb, g.M, g.out_sm, g.Cbb)) = v;
                }
            }
        }
        __syncthreads();            // the stores have read the staging tile / Gt is free: the next tile may overwrite both
    }
    // partial weight gradient of this workgroup: added to its slab
#pragma unroll
    for (int v = 0; v < NWT; ++v) {
        const int tau = wave + NWAVE * v, ib = tau & 3, jb = tau >> 2;
        if (jb < NJB) {
            float* sl = f.slab + (int64_t)blockIdx.x * f.Kt * G4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < f.Kt) sl[(int64_t)row * G4 + 32 * jb + l32] += accw[v][r];
            }
        }
    }
    block_param_reduce_n<LPN, NWAVE, 11>(pacc, h, sm, part_row, g.accumulate);
}

}  // namespace

// Launches KERNEL<NT, h / 4> (hidden 8 / 16: the entries' check comes first) for nt 32-column tiles, NT = nt clamped to the
// instances that exist: NT_LO .. NT_HI8 at hidden 8, NT_LO .. 4 at hidden 16.
#define QT_GATE_BWD_NT_(n, LO, HI) ((n) < (LO) ? (LO) : (n) > (HI) ? (HI) : (n))
#define QT_GATE_BWD_LAUNCH_(KERNEL, n, LO, HI, LPN, grid, block, stream, arg) \
    hipLaunchKernelGGL((KERNEL<QT_GATE_BWD_NT_(n, LO, HI), LPN>), dim3(grid), dim3(block), 0, (hipStream_t)stream, arg)
#define QT_GATE_BWD_LAUNCH(KERNEL, h, nt, NT_LO, NT_HI8, grid, block, stream, arg)                          \
    switch (((h) == 16 ? 4 : 0) + ((nt) < 1 ? 1 : (nt) > 4 ? 4 : (nt))) {                                   \
        case 1: QT_GATE_BWD_LAUNCH_(KERNEL, 1, NT_LO, NT_HI8, 2, grid, block, stream, arg); break;          \
        case 2: QT_GATE_BWD_LAUNCH_(KERNEL, 2, NT_LO, NT_HI8, 2, grid, block, stream, arg); break;          \
        case 3: QT_GATE_BWD_LAUNCH_(KERNEL, 3, NT_LO, NT_HI8, 2, grid, block, stream, arg); break;          \
        case 4: QT_GATE_BWD_LAUNCH_(KERNEL, 4, NT_LO, NT_HI8, 2, grid, block, stream, arg); break;          \
        case 5: QT_GATE_BWD_LAUNCH_(KERNEL, 1, NT_LO, 4, 4, grid, block, stream, arg); break;               \
        case 6: QT_GATE_BWD_LAUNCH_(KERNEL, 2, NT_LO, 4, 4, grid, block, stream, arg); break;               \
        case 7: QT_GATE_BWD_LAUNCH_(KERNEL, 3, NT_LO, 4, 4, grid, block, stream, arg); break;               \
        default: QT_GATE_BWD_LAUNCH_(KERNEL, 4, NT_LO, 4, 4, grid, block, stream, arg); break;              \
    }

// What qt_lstm_bwd_dgrad and qt_lstm_bwd_fused check and fill alike: the cell operands with their row strides, the output
// planes and the alignment of both.  Returns the reason for a refusal (the entry reports it under its own name) or nullptr;
// g arrives value-initialised and each entry adds its own fields.
static const char* cell_bwd_args(DgradCellArgs& g, const float* gO, int ld_go, const float* gHn, int ld_gh, const float* gCn, int ld_gc,
                                 const float* gates, const float* Cprev, int ld_c, const float* wc, const float* ln, int N,
                                 const int32_t* n_dev, int h, float* gCprev, float* part, int accumulate, const float* Wrows,
                                 int Kb, int Cb, int Cbb, float* out, float* outb) {
    if (!(gates && wc && part && Wrows && out)) return "null pointer";
    if (!(h == 8 || h == 16)) return "fused for hidden sizes 8 and 16 (others: qt_lstm_bwd + qt_dense2)";
    if (!(Kb >= 1 && Cb >= 4 && Cb % 4 == 0 && Cbb >= 0 && Cbb % 4 == 0 && (Cbb == 0 || outb))) return "bad output planes";
    if (!((!gHn || ld_gh >= h) && (!gCn || ld_gc >= h) && (!gO || ld_go >= h) && ld_gh % 4 == 0 && ld_gc % 4 == 0 &&
          ld_go % 4 == 0 && ld_c % 4 == 0 && (!Cprev || ld_c >= h)))
        return "bad row stride";
    if ((((uintptr_t)Wrows | (uintptr_t)gates | (uintptr_t)out | (uintptr_t)outb) & 15) != 0) return "operands must be 16-byte aligned";
    g.gO = gO; g.gHn = gHn; g.gCn = gCn; g.gates = gates; g.Cprev = Cprev; g.wc = wc; g.ln = ln;
    g.ld_go = ld_go; g.ld_gh = ld_gh; g.ld_gc = ld_gc; g.ld_c = ld_c; g.h = h;
    g.gCprev = gCprev; g.part = part; g.accumulate = accumulate;
    g.BT = Wrows; g.M = N; g.NB = Kb * (Cb + Cbb); g.Kb = Kb; g.Cb = Cb; g.Cbb = Cbb; g.out = out; g.outb = outb; g.n_dev = n_dev;
    return nullptr;
}

extern "C" int qt_lstm_dgrad_blocks(int N) { return N <= 0 ? 0 : qt_cdiv(N, BM); }

extern "C" int qt_lstm_bwd_dgrad(const float* gO, int ld_go, const float* gHn, int ld_gh, const float* gCn, int ld_gc,
                                 const float* gates, const float* Cprev, int ld_c, const float* wc, const float* ln, int N,
                                 const int32_t* n_dev, int h, float* gG, float* gCprev, float* part, int accumulate,
                                 const float* Wrows, const void* Whi, const void* Wlo, int Kb, int Cb, int Cbb, float* out,
                                 float* outb, int out_sm, const float* gHn2, int ld_gh2, const float* add0, void* stream) {
    DgradCellArgs g = {};
    const char* why = cell_bwd_args(g, gO, ld_go, gHn, ld_gh, gCn, ld_gc, gates, Cprev, ld_c, wc, ln, N, n_dev, h, gCprev, part, accumulate,
                                    Wrows, Kb, Cb, Cbb, out, outb);
    QT_ARG(!why, why);
    QT_ARG(gG && ((uintptr_t)gG & 15) == 0, "gG must be a 16-byte aligned pointer");
    QT_ARG((!gHn2 || (ld_gh2 >= h && ld_gh2 % 4 == 0)) && (((uintptr_t)gHn2 | (uintptr_t)add0) & 15) == 0, "bad second gradient / plane-0 addend");
    QT_ARG((Whi == nullptr) == (Wlo == nullptr) && (((uintptr_t)Whi | (uintptr_t)Wlo) & 15) == 0, "Whi / Wlo come as a 16-byte aligned pair");
    const int NB = g.NB;
    QT_ARG(NB <= 128, "the output planes must fit one 128-column tile");
    if (N <= 0) return QT_OK;
    g.gG = gG;
    g.BThi = (const __bf16*)Whi; g.BTlo = (const __bf16*)Wlo;
    g.out_sm = out_sm != 0;
    g.gHn2 = gHn2; g.ld_gh2 = ld_gh2; g.add0 = add0;
    // 32-column MFMA tiles: as many as the output planes need (K' C = 80 or 96 columns take three, not four), two at the least
    QT_GATE_BWD_LAUNCH(k_dgrad_cell, h, qt_cdiv(NB, 32), 2, 4, qt_cdiv(N, BM), 256, stream, g);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_num_cus(void) {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
            n_cu = 256;         // (no device visible: the MI355X count; only sizes host-side buffers)
    }
    return n_cu;
}

extern "C" int qt_lstm_bwd_fused(const float* gO, int ld_go, const float* gHn, int ld_gh, const float* gCn, int ld_gc,
                                 const float* gates, const float* Cprev, int ld_c, const float* wc, const float* ln, int N,
                                 const int32_t* n_dev, int h, float* gCprev, float* part, int accumulate,
                                 const float* Wrows, int Kb, int Cb, int Cbb, float* out, float* outb,
                                 const float* a0, int lda0, const float* a_rest, const float* a0b, int lda0b, const float* a_restb,
                                 int Ka, int Ca, int Cab, const float* S, int Ks, float* slab, int nslab, void* stream) {
    CellBwdFusedArgs f = {};
    const char* why = cell_bwd_args(f.d, gO, ld_go, gHn, ld_gh, gCn, ld_gc, gates, Cprev, ld_c, wc, ln, N, n_dev, h, gCprev, part, accumulate,
                                    Wrows, Kb, Cb, Cbb, out, outb);
    QT_ARG(!why, why);
    QT_ARG(slab && ((uintptr_t)slab & 15) == 0, "slab must be a 16-byte aligned pointer");
    const int NB = f.d.NB;
    QT_ARG(NB <= (h == 16 ? 128 : 64), "the output planes must fit the column tiles of the launch");
    if (int rc = plane_src(&f.A, __func__, a0, lda0, a_rest, a0b, lda0b, a_restb, Ka, Ca, Cab, S, Ks, N)) return rc;
    f.Kt = Ka * (Ca + Cab) + Ks;
    QT_ARG(f.Kt <= 128, "the weight must have at most 128 rows (one accumulator tile column per wave)");
    const int NTc = qt_cdiv(NB, 32);
    // 64-row tiles, two 256-thread workgroups per CU (their LDS fits twice up to three column tiles); else 128-row tiles
    const bool small = fused_tile_rows(NTc) == 64;
    const int grid = small ? min(2 * qt_num_cus(), qt_cdiv(N, 64)) : min(qt_num_cus(), qt_cdiv(N, 128));
    QT_ARG(nslab >= grid, "slab too small: one (Kt, 4h) slab per workgroup, qt_lstm_fused_blocks() of them");
    if (N <= 0) return QT_OK;
    f.slab = slab;
    QT_GATE_BWD_LAUNCH(k_cell_bwd_fused, h, NTc, 1, 2, grid, 4 * fused_tile_rows(NTc), stream, f);      // (hidden 8: NB <= 64, two tiles)
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_lstm_fused_blocks(void) { return 2 * qt_num_cus(); }

extern "C" int qt_dense_lstm(const float* a0, int lda0, const float* a_rest, const float* a0b, int lda0b, const float* a_restb,
                             int Ka, int Ca, int Cab, const float* W, const float* WT, const float* S, int Ks,
                             const float* Ws, int h, int N, const int32_t* n_dev, const float* Cprev, int ld_c,
                             const float* wc, const float* b, const float* ln, float* O, float* Hn, float* Cn,
                             float* gates, int planes_sm, void* stream) {
    QT_ARG((W || WT) && wc && b && Hn && Cn && gates, "bad arguments");
    QT_ARG(h == 8 || h == 16 || h == 32, "the fused gate GEMM + cell covers hidden sizes 8, 16 and 32 (qt_dense + qt_lstm_fwd otherwise)");
    QT_ARG((Ks == 0) || Ws || WT, "Ws missing");
    QT_ARG(Ks == 0 || WT || Ws == W + (int64_t)Ka * (Ca + Cab) * 4 * h, "Ws must follow W contiguously ([W ; Ws] is one matrix)");
    QT_ARG((((uintptr_t)W | (uintptr_t)WT | (uintptr_t)Cprev) & 15) == 0 && ld_c % 4 == 0, "operands must be 16-byte aligned");
    GemmArgs g = {};
    if (int rc = plane_src(&g.A, __func__, a0, lda0, a_rest, a0b, lda0b, a_restb, Ka, Ca, Cab, S, Ks, N, planes_sm)) return rc;
    if (N <= 0) return QT_OK;
    g.B = W; g.BT = WT; g.M = N; g.K = Ka * (Ca + Cab) + Ks; g.NB = 4 * h;
    g.Kb = 1; g.Cb = 4 * h; g.n_dev = n_dev;
    g.Cprev = Cprev; g.wc = wc; g.bias = b; g.ln = ln; g.ld_c = ld_c; g.h = h;
    g.O = O; g.Hn = Hn; g.Cn = Cn; g.gates = gates;
    // hidden 8 / 16 with the whole W^T in LDS: the persistent wave-centric kernel (one workgroup per CU)
    if ((h == 8 || h == 16) && g.K <= GATE_P_MAXK) {
        const int pitch = g.K + (((g.K >> 2) & 1) ? 8 : 4);                 // pitch / 4 odd
        const int n_cu = qt_num_cus();
        const dim3 pgrid(min(n_cu, qt_cdiv(N, 32)), 1, 1);
        const int nj = (g.K + 7) >> 3;
#define QT_GATE_P(NT_, LPN_)                                                                                              \
        do {                                                                                                              \
            if (nj == 8) hipLaunchKernelGGL((k_gate_cell_p<NT_, LPN_, 8>), pgrid, dim3(512), 0, (hipStream_t)stream, g, pitch);       \
            else if (nj == 11) hipLaunchKernelGGL((k_gate_cell_p<NT_, LPN_, 11>), pgrid, dim3(512), 0, (hipStream_t)stream, g, pitch); \
            else if (nj == 13) hipLaunchKernelGGL((k_gate_cell_p<NT_, LPN_, 13>), pgrid, dim3(512), 0, (hipStream_t)stream, g, pitch); \
            else hipLaunchKernelGGL((k_gate_cell_p<NT_, LPN_, 0>), pgrid, dim3(512), 0, (hipStream_t)stream, g, pitch);               \
        } while (0)
        if (h == 16) QT_GATE_P(2, 4);
        else QT_GATE_P(1, 2);
#undef QT_GATE_P
        QT_LAUNCHED();
        return QT_OK;
    }
    gemm_fwd_cell_launch(&g, N, (hipStream_t)stream);        // hidden 32, or a reduction too long for the persistent kernel's LDS
    QT_LAUNCHED();
    return QT_OK;
}
