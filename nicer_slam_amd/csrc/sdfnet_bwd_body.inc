// sdfnet_bwd_body.inc -- the body of k_sdfnet_bwd<L, C, NH, MAP> (render_sdfnet.hip), textually included by that kernel and by the
// two-phase kernel k_colour_coarse_bwd (render_colour.hip).  Expects in scope: SdfNetArgs a, GridGeom16 geom, float* stage
// (2 x kStageFloats floats), constexpr L, C, NH, MAP, `using P = SdfPack<NH>`, `using Seq = SdfOps<NH, true>`.
// NSA_BODY_HANDOFF (set by k_colour_coarse_bwd): the cotangents are in scope as ho_n / ho_fb / ho_gx -- what the colour phase has just
// stored to a.g_grad / a.g_feat / a.g_x for this lane's point (all three given and accumulate == 1 there) -- and are not read back.
#ifdef NSA_BODY_HANDOFF
#define NSA_COT_N(d_) ho_n[d_]
#define NSA_COT_F(q_) ho_fb[q_]
#define NSA_COT_X(d_) ho_gx[d_]
#else
#define NSA_COT_N(d_) (a.g_grad ? a.g_grad[(size_t)q * 3 + (d_)] : 0.0f)
#define NSA_COT_F(q_) (a.g_feat ? a.g_feat[(size_t)tile * 32 * 64 + lane + (q_) * 64] : 0.0f)
#define NSA_COT_X(d_) a.g_x[(size_t)q * 3 + (d_)]
#endif
    stage_begin<Seq>(stage, a.wp);
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
    float x[3], z;
    uint32_t ray;
    load_point(a.src, q, x, ray, z);
    // Kernels that run one workgroup per CU (the fine network; the MAP variants) have LDS to spare: keep the grid
    // Jacobian of this lane's levels there and skip the second and third corner gather of the backward.
    constexpr bool kJacLds = (NH > 1) || MAP;
    __shared__ float jac_lds[kJacLds ? 4 * (L / 2) * 3 * C * 64 : 1];
    float* jstore = kJacLds ? jac_lds + (threadIdx.x >> 6) * ((L / 2) * 3 * C * 64) + lane : nullptr;
    // Without the LDS Jacobian (two workgroups per CU) the grid slots of the tangent input come from the rows gathered for the
    // recompute: they need the rows, the blend weights and nbar, nothing the network produces -- one corner gather and one locate
    // per level fewer.  They wait for the tangent sweep in the part of the stage buffers that the staged fragments leave free
    // (kLdsPieces of 3 fragments are staged): level jl of this lane's two in the tail of buffer jl, 64 * C floats per wave.
    constexpr int kStageUsed = kStageFloats / 3 * kLdsPieces;
    constexpr bool kTanHead = !kJacLds && L / 2 <= 2 && kStageFloats - kStageUsed >= NSA_BODY_NW * 64 * C;
    float* tcol = stage + kStageUsed + (threadIdx.x >> 6) * (64 * C) + lane;
    // the cotangents of the outputs: there they are requested with the point, ahead of the gather that nbar then joins; the other
    // kernels are at their register cap and load them after the reverse pass
    float nbar[3], sbar = 0.0f;
    if (kTanHead) {
#pragma unroll
        for (int d = 0; d < 3; ++d) nbar[d] = NSA_COT_N(d);
        sbar = a.g_sdf ? a.g_sdf[q] : 0.0f;
    }
    float in[SDF_IN_STEPS];
    if (kTanHead) sdf_net_inputs_tangent<L, C>(x, a.divide_factor, a.table, geom, h, nbar, in, tcol, kStageFloats);
    else          sdf_net_inputs<L, C>(x, a.divide_factor, a.table, geom, h, in, jstore);
    using E = SE<NH>;
    const bool emit = MAP && a.emit != nullptr && wave_live;   // (a clamped wave must not touch the last tile's rows)
    const Emitter em{emit ? a.emit + (size_t)tile * 32 + (lane & 31) : nullptr, a.emit_ld, live};
    float sg[NH][HS], hl[HS];
    hidden_forward<NH, Seq>(stage, 0, a.wp, lane, h, in, sg, hl, emit ? &em : nullptr);
    float dh[NH > 1 ? NH - 1 : 1][HS], dl[48];
    reverse_pass<NH, Seq>(stage, NH, a.wp, lane, h, sg, dh, dl, emit ? &em : nullptr);
    if (emit) {
#pragma unroll
        for (int s = 0; s < SDF_IN_STEPS; ++s) em.slot(E::H0, s, h, in[s]);
    }

    if (!kTanHead) {
#pragma unroll
        for (int d = 0; d < 3; ++d) nbar[d] = NSA_COT_N(d);
        sbar = a.g_sdf ? a.g_sdf[q] : 0.0f;
    }

    // ---- tangent sweep: e_k = sp''(a_k) dh_k ta_k (kept in e[k-1]) ----
    float e[NH][HS];
    float emax[NH];             // (form 2 scale hints) this lane's largest |e_k|: |sg acc + e| <= |acc| + |e|
    float xb2[3];
    {
        float tin[SDF_IN_STEPS];
        if (kJacLds) tangent_from_jac<L, C>(a.divide_factor, jstore, h, in, nbar, dl, tin, xb2);
        else if (kTanHead) {
            pe_tangent(h, in, nbar, dl, tin, xb2);
            grid_tangent_slots<L, C>(tcol, kStageFloats, tin);
        } else x_to_slots_tangent<L, C>(x, a.divide_factor, a.table, geom, h, in, nbar, dl, tin, xb2);
        if (emit) {
#pragma unroll
            for (int s = 0; s < SDF_IN_STEPS; ++s) em.slot(E::TIN, s, h, tin[s]);
        }
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        gemm_staged<Seq, SDF_IN_STEPS, 2>(stage, a.wp, 2 * NH, lane, tin, acc);
        f32x16 ws[2];
        load_vec<2>(a.wp + P::kWSDF, h, ws);
        float th[HS];
#pragma unroll
        for (int k = 1; k <= NH; ++k) {
            const float bound = acc_abs_max<2>(acc);         // (form 2 scale hint: |th| <= |ta|, the Softplus derivative is a sigmoid)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = 16 * t + r;
                    const float s1 = sg[k - 1][q];
                    const float s2 = 100.0f * s1 * (1.0f - s1);          // 0 in the linear region (s1 == 1)
                    const float dhk = (k == NH) ? ws[t][r] : dh[k - 1][q];
                    e[k - 1][q] = s2 * dhk * acc[t][r];
                    th[q] = s1 * acc[t][r];
                    if (emit) em.hid(E::TH(k), q, h, th[q]);
                }
            emax[k - 1] = abs_max<HS>(e[k - 1]);
            if (k < NH) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
                gemm_staged<Seq, HS, 2>(stage, a.wp, 2 * NH + k, lane, th, acc, &bound);
            }
        }
    }
    // ---- reverse sweep ----
    float ab[HS];
    float ab_bound;             // >= this lane's largest |ab| (the next GEMM takes its scale from it)
    {
        float fb[HS];
#pragma unroll
        for (int j = 0; j < HS; ++j) fb[j] = NSA_COT_F(j);
        if (emit) {
#pragma unroll
            for (int q = 0; q < HS; ++q) em.hid(E::FB, q, h, fb[q]);
        }
        f32x16 acc[2], ws[2];
        load_vec<2>(a.wp + P::kWSDF, h, ws);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = sbar * ws[t][r];
        gemm_staged<Seq, HS, 2>(stage, a.wp, 3 * NH, lane, fb, acc);
        ab_bound = acc_abs_max<2>(acc) + emax[NH - 1];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) ab[16 * t + r] = sg[NH - 1][16 * t + r] * acc[t][r] + e[NH - 1][16 * t + r];
    }
#pragma unroll
    for (int k = NH - 1; k >= 1; --k) {
        if (emit) {
#pragma unroll
            for (int q = 0; q < HS; ++q) em.hid(E::AB(k + 1), q, h, ab[q]);
        }
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        gemm_staged<Seq, HS, 2>(stage, a.wp, 3 * NH + 1 + (NH - 1 - k), lane, ab, acc, &ab_bound);
        ab_bound = acc_abs_max<2>(acc) + emax[k - 1];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) ab[16 * t + r] = sg[k - 1][16 * t + r] * acc[t][r] + e[k - 1][16 * t + r];
    }
    if (emit) {
#pragma unroll
        for (int q = 0; q < HS; ++q) em.hid(E::AB(1), q, h, ab[q]);
    }
    float hb0[48];
    {
        f32x16 a3[3];
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) a3[t][r] = 0.0f;
        gemm_staged<Seq, HS, 3>(stage, a.wp, 4 * NH, lane, ab, a3, &ab_bound);
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) hb0[16 * t + r] = a3[t][r];
    }
    float gx[3];
    if (kJacLds) slots_to_x_jac<L, C>(a.divide_factor, jstore, h, in, hb0, gx);
    else         slots_to_x<L, C>(x, a.divide_factor, a.table, geom, h, in, hb0, gx);
    // scatter scratch: the stage buffer the last GEMM (op 4 NH, even) does NOT read; every wave passed the barrier of
    // that GEMM, so nobody reads it any more
    if (MAP && a.g_table)
        table_grad_scatter<L, C>(x, a.divide_factor, geom, h, lane, live, hb0, dl, nbar, a.g_table,
                                 stage + kStageFloats + (threadIdx.x >> 6) * 64 * (2 * C + 1));
#pragma unroll
    for (int d = 0; d < 3; ++d) gx[d] = xhalf_sum(gx[d] + xb2[d]);
    if (live && h == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float v = gx[d];
            if (a.accumulate) v += NSA_COT_X(d);
            a.g_x[(size_t)q * 3 + d] = v;
        }
    }
#undef NSA_COT_N
#undef NSA_COT_F
#undef NSA_COT_X
