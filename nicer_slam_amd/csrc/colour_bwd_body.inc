// colour_bwd_body.inc -- the body of k_colour_bwd<MAP> (render_colour.hip), textually included by that kernel and by the
// two-phase kernel k_colour_coarse_bwd (same file) so that both compile the same statements.  Expects in scope: ColourArgs a,
// GridGeom16 geom, float* stage (2 x kColStage floats at least), `using Seq = ColBwdOps<MAP>`, a constexpr/template bool MAP.
    stage_issue_op(a.wp, Seq::op(0), stage);
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    uint32_t tile = blockIdx.x * NSA_BODY_NW + (threadIdx.x >> 6);
    const uint32_t n_tiles = (a.src.P + 31) / 32;
    const bool wave_live = tile < n_tiles;
    if (!wave_live) tile = n_tiles - 1;
    uint32_t pid = tile * 32 + (lane & 31);
    const bool live = wave_live && pid < a.src.P;
    if (pid >= a.src.P) pid = a.src.P - 1;
    const uint32_t q = point_of(a.src, pid);                // point handled by this lane pair
    float x[3], z, dir[3];
    uint32_t ray;
    load_point(a.src, q, x, ray, z);
#pragma unroll
    for (int d = 0; d < 3; ++d) dir[d] = a.src.rays_d[ray * 3 + d];
    // MAP: the mapping form recomputes the forward (its activations are emission rows of the weight gradients).
    // !MAP: the data-path form takes the ReLU masks and the sigmoid outputs from the forward's save-area extension (save_ext): no
    // first-layer input vector, no recomputation -- three staged parts instead of six (round 5; the recomputation was 42 % and the
    // input fetch 16 % of this phase's cycles, profiles/r04_ab_experiments.txt r4n).
    float in[COL_IN_STEPS];                                  // (MAP only; dead otherwise)
    float pe_s[6], pe_c[6];                                  // sin / cos of 2^k dir_d of this lane's pairs (d/d dir below)
    f32x16 a1[2], a2[2];
    float rgb[3];
    uint32_t mask1 = 0, mask2 = 0;
    if constexpr (MAP) {
        colour_inputs(a, geom, tile, q, lane, h, x, dir, in, true, wave_live);
#pragma unroll
        for (int j = 0; j < 6; ++j) { pe_s[j] = in[37 + 2 * j]; pe_c[j] = in[38 + 2 * j]; }
        CTS_MARK(4)
        colour_mlp<Seq, true>(stage, a.wp, lane, h, in, a1, a2, rgb);
    } else {
        const float* ext = save_ext(a.save, a.src.P, tile);
        mask1 = __float_as_uint(ext[lane]);
        mask2 = __float_as_uint(ext[64 + lane]);
#pragma unroll
        for (int j = 0; j < 3; ++j) rgb[j] = ext[128 + 32 * j + (lane & 31)];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int g0 = 2 * j, g1 = 2 * j + 1;
            const float da = h ? dir[g1 % 3] : dir[g0 % 3];
            const float sc = h ? (float)(1 << (g1 / 3)) : (float)(1 << (g0 / 3));
            sincos_f(da * sc, pe_s[j], pe_c[j]);
        }
        CTS_MARK(4)
    }
    CTS_MARK(5)
    const bool emit = MAP && a.emit != nullptr && wave_live;
    const ColEmitter em{emit ? a.emit + (size_t)tile * 32 + (lane & 31) : nullptr, a.emit_ld, live};
    if constexpr (MAP) {
        if (emit) {
#pragma unroll
            for (int s = 0; s < COL_IN_STEPS; ++s) em.slot(CE_IN, s, h, in[s]);
#pragma unroll
            for (int q = 0; q < HS; ++q) {
                em.hid(CE_H1, q, h, relu_f(a1[q >> 4][q & 15]));
                em.hid(CE_H2, q, h, relu_f(a2[q >> 4][q & 15]));
            }
        }
    }
    // d/d(pre-sigmoid), d/d h2 = sum_j ob_j W2[j,:], relu masks (torch: grad * (a > 0))
    float ab[HS];
    {
        float ob[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) ob[j] = a.g_rgb[(size_t)q * 3 + j] * rgb[j] * (1.0f - rgb[j]);
        if (emit && h == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) em.base[(size_t)(CE_OB + j) * em.ld] = live ? ob[j] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < HS; ++q) ab[q] = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            f32x16 wv[2];
            load_vec<2>(a.wp + ColPack::kW2V + 64 * j, h, wv);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) ab[16 * t + r] = fmaf(ob[j], wv[t][r], ab[16 * t + r]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool on = MAP ? a2[t][r] > 0.0f : ((mask2 >> (16 * t + r)) & 1u) != 0u;
                ab[16 * t + r] = on ? ab[16 * t + r] : 0.0f;
            }
    }
    if (emit) {
#pragma unroll
        for (int q = 0; q < HS; ++q) em.hid(CE_AB2, q, h, ab[q]);
    }
    CTS_MARK(6)
    float m_ab = 0.0f;
    {
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        gemm_staged_part<Seq, kColStage, HS, 2, 0, 4>(stage, a.wp, Seq::kRev, lane, ab, acc);
        m_ab = acc_abs_max<2>(acc);              // (form 2 scale hint for the next GEMM: a masked value is at most |acc|)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool on = MAP ? a1[t][r] > 0.0f : ((mask1 >> (16 * t + r)) & 1u) != 0u;
                ab[16 * t + r] = on ? acc[t][r] : 0.0f;
            }
    }
    if (emit) {
#pragma unroll
        for (int q = 0; q < HS; ++q) em.hid(CE_AB1, q, h, ab[q]);
    }
    CTS_MARK(7)
    float ib[80];
    {
        f32x16 a5[5];
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) a5[t][r] = 0.0f;
        gemm_staged_part<Seq, kColStage, HS, 5, 0, 2, true, false>(stage, a.wp, Seq::kRev + 1, lane, ab, a5, &m_ab);   // (one scale, one
        gemm_staged_part<Seq, kColStage, HS, 5, 2, 2, false, true>(stage, a.wp, Seq::kRev + 2, lane, ab, a5, &m_ab);   //  scaling of a5)
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) ib[16 * t + r] = a5[t][r];
    }
    CTS_MARK(8)
    // feature cotangent -> HL
    float* fdst = a.g_feat + (size_t)tile * 32 * 64 + lane;
    if (wave_live) {
#pragma unroll
        for (int q = 0; q < HS; ++q) fdst[q * 64] = ib[q];
    }
    // scalar slots
    float gx[3], gd[3], gg[3];
    gx[0] = h ? 0.0f : ib[32];   gx[1] = h ? ib[32] : 0.0f;   gx[2] = h ? 0.0f : ib[33];
    gd[0] = h ? ib[33] : 0.0f;   gd[1] = h ? 0.0f : ib[34];   gd[2] = h ? ib[34] : 0.0f;
    gg[0] = h ? 0.0f : ib[35];   gg[1] = h ? ib[35] : 0.0f;   gg[2] = h ? 0.0f : ib[36];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int g0 = 2 * j, g1 = 2 * j + 1;
        const float sc = h ? (float)(1 << (g1 / 3)) : (float)(1 << (g0 / 3));
        const float t = sc * (pe_c[j] * ib[37 + 2 * j] - pe_s[j] * ib[38 + 2 * j]);
        gd[g0 % 3] += h ? 0.0f : t;
        gd[g1 % 3] += h ? t : 0.0f;
    }
    CTS_MARK(9)
    if (a.grid_grad) {   // x += J^T fbar / (2 df) with the Jacobian saved by the forward pass
        const float* sv = a.save + (size_t)tile * 64 * 64 + lane;
        const float chain = 1.0f / (2.0f * a.divide_factor);
#pragma unroll
        for (int jl = 0; jl < CL / 2; ++jl)
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int c = 0; c < CC; ++c)
                    gx[d] = fmaf(sv[(16 + (jl * 3 + d) * CC + c) * 64] * chain, ib[49 + jl * CC + c], gx[d]);
    }
    CTS_MARK(10)
    if (MAP && a.grid_grad && a.g_table) {   // colour-table gradient: w_corner * fbar, run-merged (kernel_grid_backward)
        float u[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) u[d] = to_unit(x[d], a.divide_factor);
#pragma unroll
        for (int jl = 0; jl < CL / 2; ++jl) {
            const LevelGeom lg = geom.lv[2 * jl + h];
            uint32_t cell[3];
            float w[3], dw[3];
            const bool active = locate<3>(u, lg.scale, cell, w, dw) && live;
            // scratch: stage buffer 0 -- the last GEMM part (op 5, odd) reads buffer 1, and every wave is past op 4
            float* tile = stage + (threadIdx.x >> 6) * 64 * (2 * CC + 1);
            uint32_t row[8];
            float wt8[8];
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                float wt = 1.0f;
                uint32_t q[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int bit = (corner >> d) & 1;
                    wt *= bit ? w[d] : 1.0f - w[d];
                    q[d] = cell[d] + bit;
                }
                row[corner] = lg.row0 + level_row<3>(lg, q);
                wt8[corner] = wt;
            }
            // x-neighbour corners leave as one 16-byte span wherever they are adjacent rows (dense levels; even cells of hashed ones)
#pragma unroll
            for (int yz = 0; yz < 4; ++yz) {
                float v0[CC], v1[CC];
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    v0[c] = wt8[2 * yz] * ib[49 + jl * CC + c];
                    v1[c] = wt8[2 * yz + 1] * ib[49 + jl * CC + c];
                }
                scatter_x_pair<CC>(a.g_table, row[2 * yz], row[2 * yz + 1], active, v0, v1, lane, tile);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { gx[d] = xhalf_sum(gx[d]); gd[d] = xhalf_sum(gd[d]); gg[d] = xhalf_sum(gg[d]); }
#ifdef NSA_BODY_HANDOFF
    // two-phase kernel: the next phase takes the feature cotangent, the updated normal cotangent and d/dx from these registers.
    // Every lane forms the sum its pair's first lane stores (a clamped lane the one of the point it repeats): same operands, same bits.
#pragma unroll
    for (int j = 0; j < HS; ++j) ho_fb[j] = ib[j];
#pragma unroll
    for (int d = 0; d < 3; ++d) { ho_gx[d] = gx[d]; ho_n[d] = a.g_grad[(size_t)q * 3 + d] + gg[d]; }
#endif
    if (live && h == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a.g_x[(size_t)q * 3 + d] = gx[d];
            a.g_dir[(size_t)q * 3 + d] = gd[d];
#ifdef NSA_BODY_HANDOFF
            a.g_grad[(size_t)q * 3 + d] = ho_n[d];
#else
            a.g_grad[(size_t)q * 3 + d] += gg[d];
#endif
        }
    }
