// sdfnet4_bwd_body.inc -- one 16-point tile of k_sdfnet4_bwd<L, C, NH, MAP> (render_sdfnet4.hip), textually included by that kernel and
// by its resident-weight persistent form k_sdfnet4_bwd_res (bf16-operand build, data path) so that both compile the same statements.
// Expects in scope: SdfNet4Args a, float* stage (stage buffers resp. resident image), LevelGeom s_geom[16], lane, j, q, tile, wave_live,
// `using P, Seq, E`, the template parameters L, C, NH, MAP and the macro NSA_BODY_SYNC.
    uint32_t pid = tile * 16 + j;
    const bool live = wave_live && pid < a.src.P;
    if (pid >= a.src.P) pid = a.src.P - 1;
    const uint32_t pt = point_of(a.src, pid);
    float x[3], z;
    uint32_t ray;
    load_point(a.src, pt, x, ray, z);
    // The data path of the fp32 build (Seq = SdfOps4Data, render_sdfnet4.hip) runs forward with tangent sweep and reverse pass with
    // reverse sweep, two operands per staged block; the tangent input is formed at the head, so nbar is requested with the point.
    constexpr bool kPaired = !MAP && kPairedBwd4;
    float nbar[3], sbar = 0.0f;
    if constexpr (kPaired) {
#pragma unroll
        for (int d = 0; d < 3; ++d) nbar[d] = a.g_grad ? a.g_grad[(size_t)pt * 3 + d] : 0.0f;
        sbar = a.g_sdf ? a.g_sdf[pt] : 0.0f;
    }
    NSA_BODY_SYNC                                            // s_geom (staged form: every tile; resident form: once, before the loop)
    TS_MARK(4)
    // the grid Jacobian of this lane's levels stays in lane-private LDS: the backward needs no second and third corner gather
    constexpr int kJac = (8 / C) * 3 * C;                    // 24 floats per lane
    __shared__ float jac_lds[Seq::NW * kJac * 64];
    float* jstore = jac_lds + (threadIdx.x >> 6) * (kJac * 64) + lane;
    float in[QIN];
    pe_slots4(x, q, in);
    grid_slots4<L, C>(x, a.divide_factor, a.table, s_geom, q, in, jstore);
    const bool emit = MAP && a.emit != nullptr && wave_live;   // (a clamped wave must not touch the last tile's rows)
    const Emitter4 em{emit ? a.emit + (size_t)tile * 16 + j : nullptr, a.emit_ld, live};
    float dl[QIN], hb0[QIN], xb2[3];
    if constexpr (kPaired) {
        // Every product, every accumulation order, every scale and hint is the unpaired branch's below: the results are bit for bit
        // those of the MAP kernel's data outputs.
        // ---- forward | tangent: h_k = sp(a_k), th_k = sp'(a_k) ta_k, layer by layer through the same block ----
        float sg[NH][QHS], ta[NH][QHS];                      // ta_k is kept (not e_k): dh_k does not exist yet
        TS_MARK(5)
        {
            float tin[QIN];
            tangent_tin_from_jac4<L, C>(a.divide_factor, jstore, q, in, nbar, tin);
            f32x4v acc[4], tac[4];
            load_vec16(a.wp + P::kB0, q, acc);
            zero16(tac, 4);
            gemm16_staged2<Seq, Seq::NW, Seq::BUF, QIN_G, 4>(stage, a.wp, 0, lane, in, acc, tin, tac);
            float hl[QHS], th[QHS];
#pragma unroll
            for (int k = 1; k <= NH; ++k) {
                float d2;
                const float bound = acc_abs_max16<4>(acc) + kSoftplusSlack;
                const float tbound = acc_abs_max16<4>(tac);      // (|th| <= |ta|: the Softplus derivative is a sigmoid)
#pragma unroll
                for (int s = 0; s < QHS; ++s) {
                    softplus100_all(acc[s >> 2][s & 3], hl[s], sg[k - 1][s], d2);
                    ta[k - 1][s] = tac[s >> 2][s & 3];
                    th[s] = sg[k - 1][s] * ta[k - 1][s];
                }
                if (k < NH) {
                    load_vec16(a.wp + P::bh(k), q, acc);
                    zero16(tac, 4);
                    gemm16_staged2<Seq, Seq::NW, Seq::BUF, 2, 4>(stage, a.wp, k, lane, hl, acc, th, tac, &bound, &tbound);
                }
            }
        }
        TS_MARK(6)
        // ---- WFEAT^T (unshared): ab_NH = sp'(a_NH) (sbar wsdf + WFEAT^T fb) + e_NH; da_NH = sp'(a_NH) wsdf ----
        float da[QHS], ab[QHS];
        float ab_bound;             // >= this lane's largest |ab| (the next GEMM takes its scale from it)
        {
            float fb[QHS];
            const float* fsrc = a.g_feat ? a.g_feat + hl_base4(tile, j, q) : nullptr;
#pragma unroll
            for (int s = 0; s < QHS; ++s) fb[s] = fsrc ? fsrc[hl_step4(s)] : 0.0f;
            f32x4v acc[4], ws[4];
            load_vec16(a.wp + P::kWSDF, q, ws);
#pragma unroll
            for (int t = 0; t < 4; ++t)        // (element by element: a vector * scalar here becomes v_pk_mul_f32, see build.py::isa_check)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][r] = sbar * ws[t][r];
            gemm16_staged<Seq, Seq::NW, Seq::BUF, 2, 4>(stage, a.wp, NH, lane, fb, acc);
            float e[QHS];
#pragma unroll
            for (int s = 0; s < QHS; ++s) {
                const float s1 = sg[NH - 1][s];
                const float s2 = 100.0f * s1 * (1.0f - s1);          // 0 in the linear region (s1 == 1)
                e[s] = s2 * ws[s >> 2][s & 3] * ta[NH - 1][s];
                da[s] = s1 * ws[s >> 2][s & 3];
            }
            ab_bound = acc_abs_max16<4>(acc) + abs_max<QHS>(e);
#pragma unroll
            for (int s = 0; s < QHS; ++s) ab[s] = sg[NH - 1][s] * acc[s >> 2][s & 3] + e[s];
        }
        TS_MARK(7)
        // ---- reverse pass | reverse sweep: (da_{k+1}, ab_{k+1}) x W_k^T -> dh_k -> e_k -> (da_k, ab_k) ----
        float da_bound = 0.0f;
        const float* da_hint = nullptr;
#pragma unroll
        for (int k = NH - 1; k >= 1; --k) {
            f32x4v acc[4], bac[4];
            zero16(acc, 4);
            zero16(bac, 4);
            gemm16_staged2<Seq, Seq::NW, Seq::BUF, 2, 4>(stage, a.wp, NH + 1 + (NH - 1 - k), lane, da, acc, ab, bac, da_hint, &ab_bound);
            da_bound = acc_abs_max16<4>(acc);                // |da| <= |acc|: the Softplus derivative is a sigmoid
            da_hint = &da_bound;
            float e[QHS];
#pragma unroll
            for (int s = 0; s < QHS; ++s) {
                const float s1 = sg[k - 1][s];
                const float s2 = 100.0f * s1 * (1.0f - s1);
                const float dhk = acc[s >> 2][s & 3];
                e[s] = s2 * dhk * ta[k - 1][s];
                da[s] = s1 * dhk;
            }
            ab_bound = acc_abs_max16<4>(bac) + abs_max<QHS>(e);
#pragma unroll
            for (int s = 0; s < QHS; ++s) ab[s] = sg[k - 1][s] * bac[s >> 2][s & 3] + e[s];
        }
        TS_MARK(8)
        {
            f32x4v a6[6], b6[6];
            zero16(a6, 6);
            zero16(b6, 6);
            gemm16_staged2<Seq, Seq::NW, Seq::BUF, 2, 6>(stage, a.wp, 2 * NH, lane, da, a6, ab, b6, da_hint, &ab_bound);
#pragma unroll
            for (int s = 0; s < QIN; ++s) {
                dl[s] = a6[s >> 2][s & 3];
                hb0[s] = b6[s >> 2][s & 3];
            }
        }
        pe_tangent_xbar4(q, in, nbar, dl, xb2);
        TS_MARK(9)
    } else {
        float sg[NH][QHS], hl[QHS];
        TS_MARK(5)
        hidden_forward4<NH, Seq>(stage, 0, a.wp, lane, q, in, sg, hl, emit ? &em : nullptr);
        TS_MARK(6)
        float dh[NH > 1 ? NH - 1 : 1][QHS];
        reverse_pass4<NH, Seq>(stage, NH, a.wp, lane, q, sg, dh, dl, emit ? &em : nullptr);
        TS_MARK(7)
        if (emit) {
#pragma unroll
            for (int s = 0; s < QIN; ++s) em.slot(E::H0, s, q, in[s]);
        }

#pragma unroll
        for (int d = 0; d < 3; ++d) nbar[d] = a.g_grad ? a.g_grad[(size_t)pt * 3 + d] : 0.0f;
        sbar = a.g_sdf ? a.g_sdf[pt] : 0.0f;

        // ---- tangent sweep: e_k = sp''(a_k) dh_k ta_k (kept in e[k-1]) ----
        float e[NH][QHS];
        float emax[NH];             // (form 2 scale hints) this lane's largest |e_k|: |sg acc + e| <= |acc| + |e|
        {
            float tin[QIN];
            tangent_from_jac4<L, C>(a.divide_factor, jstore, q, in, nbar, dl, tin, xb2);
            if (emit) {
#pragma unroll
                for (int s = 0; s < QIN; ++s) em.slot(E::TIN, s, q, tin[s]);
            }
            f32x4v acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
            gemm16_staged<Seq, Seq::NW, Seq::BUF, QIN_G, 4>(stage, a.wp, 2 * NH, lane, tin, acc);
            f32x4v ws[4];
            load_vec16(a.wp + P::kWSDF, q, ws);
            float th[QHS];
#pragma unroll
            for (int k = 1; k <= NH; ++k) {
                const float bound = acc_abs_max16<4>(acc);       // (form 2 scale hint: |th| <= |ta|, the Softplus derivative is a sigmoid)
#pragma unroll
                for (int s = 0; s < QHS; ++s) {
                    const float s1 = sg[k - 1][s];
                    const float s2 = 100.0f * s1 * (1.0f - s1);          // 0 in the linear region (s1 == 1)
                    const float dhk = (k == NH) ? ws[s >> 2][s & 3] : dh[k - 1][s];
                    const float ta = acc[s >> 2][s & 3];
                    e[k - 1][s] = s2 * dhk * ta;
                    th[s] = s1 * ta;
                    if (emit) em.hid(E::TH(k), s, q, th[s]);
                }
                emax[k - 1] = abs_max<QHS>(e[k - 1]);
                if (k < NH) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
                    gemm16_staged<Seq, Seq::NW, Seq::BUF, 2, 4>(stage, a.wp, 2 * NH + k, lane, th, acc, nullptr, &bound);
                }
            }
        }
        TS_MARK(8)
        // ---- reverse sweep ----
        float ab[QHS];
        float ab_bound;             // >= this lane's largest |ab| (the next GEMM takes its scale from it)
        {
            float fb[QHS];
            const float* fsrc = a.g_feat ? a.g_feat + hl_base4(tile, j, q) : nullptr;
#pragma unroll
            for (int s = 0; s < QHS; ++s) fb[s] = fsrc ? fsrc[hl_step4(s)] : 0.0f;
            if (emit) {
#pragma unroll
                for (int s = 0; s < QHS; ++s) em.hid(E::FB, s, q, fb[s]);
            }
            f32x4v acc[4], ws[4];
            load_vec16(a.wp + P::kWSDF, q, ws);
#pragma unroll
            for (int t = 0; t < 4; ++t)        // (element by element: a vector * scalar here becomes v_pk_mul_f32, see build.py::isa_check)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][r] = sbar * ws[t][r];
            gemm16_staged<Seq, Seq::NW, Seq::BUF, 2, 4>(stage, a.wp, 3 * NH, lane, fb, acc);
            ab_bound = acc_abs_max16<4>(acc) + emax[NH - 1];
#pragma unroll
            for (int s = 0; s < QHS; ++s) ab[s] = sg[NH - 1][s] * acc[s >> 2][s & 3] + e[NH - 1][s];
        }
#pragma unroll
        for (int k = NH - 1; k >= 1; --k) {
            if (emit) {
#pragma unroll
                for (int s = 0; s < QHS; ++s) em.hid(E::AB(k + 1), s, q, ab[s]);
            }
            f32x4v acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
            gemm16_staged<Seq, Seq::NW, Seq::BUF, 2, 4>(stage, a.wp, 3 * NH + 1 + (NH - 1 - k), lane, ab, acc, nullptr, &ab_bound);
            ab_bound = acc_abs_max16<4>(acc) + emax[k - 1];
#pragma unroll
            for (int s = 0; s < QHS; ++s) ab[s] = sg[k - 1][s] * acc[s >> 2][s & 3] + e[k - 1][s];
        }
        if (emit) {
#pragma unroll
            for (int s = 0; s < QHS; ++s) em.hid(E::AB(1), s, q, ab[s]);
        }
        TS_MARK(9)
        {
            f32x4v a6[6];
#pragma unroll
            for (int t = 0; t < 6; ++t) a6[t] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
            gemm16_staged<Seq, Seq::NW, Seq::BUF, 2, 6>(stage, a.wp, 4 * NH, lane, ab, a6, nullptr, &ab_bound);
#pragma unroll
            for (int s = 0; s < QIN; ++s) hb0[s] = a6[s >> 2][s & 3];
        }
    }
    float gx[3];
    slots_to_x_jac4<L, C>(a.divide_factor, jstore, q, in, hb0, gx);
    // scatter scratch: the stage buffer the last GEMM part does NOT read; every wave passed the barrier of that part and
    // nothing is fetched after it, so nobody touches that buffer any more
    constexpr int kIdle = (Seq::n_parts() - 1) & 1 ? 0 : 1;
    if (MAP && a.g_table)
        table_grad_scatter4<L, C>(x, a.divide_factor, s_geom, q, lane, live, hb0, dl, nbar, a.g_table,
                                  stage + kIdle * Seq::BUF + (threadIdx.x >> 6) * 64 * (2 * C + 1));
#pragma unroll
    for (int d = 0; d < 3; ++d) gx[d] = quad_sum(gx[d] + xb2[d]);
    if (live && q == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float v = gx[d];
            if (a.accumulate) v += a.g_x[(size_t)pt * 3 + d];
            a.g_x[(size_t)pt * 3 + d] = v;
        }
    }
