// forward-kernel per-q-tile body — textually included THREE times by
// attn_fwd.hip (preprocessor include, not a header), once per BodyForm; which
// instantiation takes which form, and the measurements, are at
// fwd_body_form() there:
//   * BODY_FRAME, inside a lambda passed to noinline_call (full-featured
//     PAIRED): the noinline frame confines register allocation to the body
//     (the pair loop's liveness otherwise spills 532 B/lane; measured +5%
//     causal)
//   * BODY_LAMBDA, a directly-called lambda with a value copy of the params
//     (full-featured d128 plain)
//   * BODY_DIRECT, at pit-loop scope (every LEAN instantiation; full-featured
//     d64 / d32 plain, where the SAME body via an inlined lambda costs
//     264 B/lane of scratch and -3.5% fwd-only, 454 vs 471 TF same box, and
//     via the noinline frame -12%)
// Context expected at inclusion: P (FwdParams value or reference), qtile,
// lds, tid/lane/wid/l31/lhi, b/h/hk, LEAN, and FWD_EXIT (return | continue).
//
// LEAN (constexpr bool) compiles the body WITHOUT the four cold features:
// the ticks stamps, the ablate switches, the key-pad mask and the bias.  They
// are `if constexpr (!LEAN)`, not folded run-time tests: as run-time branches
// in the tile loop they cost the d64 plain kernel 64 v_mov_b64 per tile (phi
// copies of s[] and o_acc forced by the ablate == 2 exit and the block cuts
// of the stamp branches), spills in the loop, and at d128 556 B/lane of
// scratch.  The lean body also loads full tiles without per-lane predicates
// and keeps the O rescale single-issue.  !LEAN is the code as it was,
// instruction for instruction; the launcher picks LEAN exactly when none of
// the four features is asked for.  The arithmetic of the two is the same.
#define FWD_STAMP(n)                                                          \
    if constexpr (!LEAN)                                                      \
        if (stamp) P.ticks[t * 6 + (n)] = __builtin_amdgcn_s_memtime()
    const long irow0 = (long)qtile * QROWS_WG + wid * QROWS_WAVE;  // this wave's first q row
    const long i = irow0 + l31;                                     // this lane's q row
    const bool row_valid = i < P.nq;
    const long i_clamped = row_valid ? i : 0;

    // ---- load Q fragments (bf16x8 per k-step): q[b, i, h, ks*16 + lhi*8 .. +8]
    const __bf16* qbase = (const __bf16*)P.q + ((long)b * P.nq + i_clamped) * P.h * D + (long)h * D;
    bf16x8 qf[KSTEPS];
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
        qf[ks] = *(const bf16x8*)(qbase + ks * 16 + lhi * 8);

    // ---- accumulators
    float m_run = MASK_VALUE_F;   // running row max of scaled scores (lane's q row)
    float l_run = 0.f;            // running row sum
    f32x16 o_acc[DBLK];           // O^T[d][q]: j = l31 = q, rows = d pattern
    #pragma unroll
    for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x16{};

    const bool split_mode = P.kv_split > 1;
    const int zsplit = blockIdx.z;
    if (!P.is_first && !split_mode) {   // resume from a previous ring hop
        const float* mrow = P.m + ((long)b * P.h + h) * P.nq;
        const float* lrow = P.l + ((long)b * P.h + h) * P.nq;
        m_run = mrow[i_clamped] * LOG2E;   // external contract is natural log
        l_run = lrow[i_clamped];
        const float* oa = P.o_acc + (((long)b * P.h + h) * D) * P.nq;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                o_acc[db][r] = oa[(long)d * P.nq + i_clamped];
            }
    }

    // ---- causal / lookback tile bounds for this workgroup: the masked
    // region is contiguous, so the tile range is computed once (keeps the
    // staging pipeline branch-free).  The algebra lives in attn_mask.h; q
    // positions are in kv-local coordinates.
    const Mask M = mask_of(P);
    const long wg_i_min = (long)qtile * QROWS_WG;
    const long wg_i_max = min((long)(qtile + 1) * QROWS_WG, P.nq) - 1;
    const long wg_q_min = M.qpos(wg_i_min);
    const long wg_q_max = M.qpos(wg_i_max);
    const long qpos_i = M.qpos(i);                    // this lane's q position
    TileRange tr = M.kv_tile_range(wg_i_min, wg_i_max, P.nk, KVBLK);
    // this z's share of THIS WG's valid tile range
    if (split_mode) tr = split_share(tr, P.kv_split, zsplit);
    const int t_lo = tr.lo, t_hi = tr.hi;

    // ---- T14 async-stage split: per-thread staging registers
    constexpr int CH_PER_ROW = D * 2 / 16;
    constexpr int KCHUNKS = KVBLK * CH_PER_ROW;          // K-tile 16B chunks
    constexpr int KREGS = (KCHUNKS + NTHREADS - 1) / NTHREADS;
    constexpr int VPAIRS = (KVBLK / 2) * (D / 8);
    constexpr int VREGS = (VPAIRS + NTHREADS - 1) / NTHREADS;
    const __bf16* kbase = (const __bf16*)P.k + ((long)b * P.nk) * P.hk * D + (long)hk * D;
    const __bf16* vbase = (const __bf16*)P.v + ((long)b * P.nk) * P.hk * D + (long)hk * D;
    const unsigned char* mbase = nullptr;
    if constexpr (!LEAN)
        mbase = P.kmask ? (const unsigned char*)P.kmask + (long)b * P.nk : nullptr;

    uint4 kst[KREGS];
    bf16x8 vsta[VREGS], vstb[VREGS];
    unsigned char mst = 1;

    // running per-thread source pointers: load_tile is always called for
    // consecutive tiles, so addresses advance by a constant — no per-tile
    // 64-bit multiplies in the hot loop
    const long kv_row_stride = (long)P.hk * D;
    const long tile_stride = KVBLK * kv_row_stride;
    const __bf16* kptr = kbase + (long)t_lo * tile_stride
        + (tid / CH_PER_ROW) * kv_row_stride + (tid % CH_PER_ROW) * 8;
    const __bf16* vptra = vbase + (long)t_lo * tile_stride
        + ((tid % (KVBLK / 2)) * 2) * kv_row_stride + (tid / (KVBLK / 2)) * 8;
    const __bf16* vptrb = vptra + kv_row_stride;
    long j0_next = (long)t_lo * KVBLK;
    long j0_staged = j0_next;   // LEAN: first key of the tile in the staging registers

    auto load_tile = [&]() {
        const long j0 = j0_next;
        const long jmax = min(j0 + KVBLK, P.nk) - 1;
        const bool full = jmax - j0 == KVBLK - 1;
        if constexpr (LEAN) {
            // Every load is unconditional: a row past the end of the ragged
            // last tile reads key row 0 instead and is zeroed when the tile
            // goes to LDS (write_tile, one scalar branch).  A
            // `valid ? load : 0` here is a 64-bit v_cmp, a saveexec, a
            // branch and a zero fill around each load, on every tile.
            constexpr int KROW_STEP = NTHREADS / CH_PER_ROW;
            constexpr int VD_STEP = (NTHREADS / (KVBLK / 2)) * 8;
            #pragma unroll
            for (int r = 0; r < KREGS; ++r) {
                int c = tid + r * NTHREADS;
                if (c < KCHUNKS) {
                    const bool ok = full || (j0 + c / CH_PER_ROW) <= jmax;
                    kst[r] = *(const uint4*)(ok ? kptr + (long)(r * KROW_STEP) * kv_row_stride
                                                : kbase + (tid % CH_PER_ROW) * 8);
                }
            }
            #pragma unroll
            for (int r = 0; r < VREGS; ++r) {
                int c = tid + r * NTHREADS;
                if (c < VPAIRS) {
                    const long ja = j0 + (c % (KVBLK / 2)) * 2;
                    const __bf16* row0 = vbase + (tid / (KVBLK / 2)) * 8 + r * VD_STEP;
                    vsta[r] = *(const bf16x8*)((full || ja <= jmax) ? vptra + r * VD_STEP : row0);
                    vstb[r] = *(const bf16x8*)((full || ja + 1 <= jmax) ? vptrb + r * VD_STEP : row0);
                }
            }
            j0_staged = j0;
        } else {
            #pragma unroll
            for (int r = 0; r < KREGS; ++r) {
                int c = tid + r * NTHREADS;
                if (c < KCHUNKS) {
                    const __bf16* src = kptr + (long)(r * (NTHREADS / CH_PER_ROW)) * kv_row_stride;
                    kst[r] = (full || (j0 + c / CH_PER_ROW) <= jmax)
                             ? *(const uint4*)src : uint4{0, 0, 0, 0};
                }
            }
            #pragma unroll
            for (int r = 0; r < VREGS; ++r) {
                int c = tid + r * NTHREADS;
                if (c < VPAIRS) {
                    // extra r steps advance along d (same kv pair)
                    const __bf16* sa = vptra + r * (NTHREADS / (KVBLK / 2)) * 8;
                    const __bf16* sb = vptrb + r * (NTHREADS / (KVBLK / 2)) * 8;
                    long ja = j0 + (c % (KVBLK / 2)) * 2;
                    vsta[r] = (full || ja <= jmax) ? *(const bf16x8*)sa : bf16x8{};
                    vstb[r] = (full || ja + 1 <= jmax) ? *(const bf16x8*)sb : bf16x8{};
                }
            }
            if (mbase && tid < KVBLK)
                mst = (j0 + tid <= jmax) ? mbase[j0 + tid] : 0;
        }
        kptr += tile_stride;
        vptra += tile_stride;
        vptrb += tile_stride;
        j0_next += KVBLK;
    };

    auto write_tile = [&](int par) {
        if constexpr (LEAN) {
            const long rows = P.nk - j0_staged;      // valid rows of the staged tile
            if (rows < KVBLK) {                      // ragged last tile: the rest are 0
                #pragma unroll
                for (int r = 0; r < KREGS; ++r)
                    if ((tid + r * NTHREADS) / CH_PER_ROW >= rows) kst[r] = uint4{0, 0, 0, 0};
                #pragma unroll
                for (int r = 0; r < VREGS; ++r) {
                    const int la = ((tid + r * NTHREADS) % (KVBLK / 2)) * 2;
                    if (la >= rows) vsta[r] = bf16x8{};
                    if (la + 1 >= rows) vstb[r] = bf16x8{};
                }
            }
        }
        #pragma unroll
        for (int r = 0; r < KREGS; ++r) {
            int c = tid + r * NTHREADS;
            if (c < KCHUNKS) {
                int row = c / CH_PER_ROW, ch = c % CH_PER_ROW;
                *(uint4*)(lds.k[par] + row * D + swz<D / 8>(row, ch) * 8) = kst[r];
            }
        }
        #pragma unroll
        for (int r = 0; r < VREGS; ++r) {
            int c = tid + r * NTHREADS;
            if (c < VPAIRS) {
                // kv pairs land in the PV k order (kperm_pair): the packed P
                // pairs are then the B fragments with no lane exchange
                int jp = kperm_pair(c % (KVBLK / 2));
                int d0 = (c / (KVBLK / 2)) * 8;
                #pragma unroll
                for (int e = 0; e < 8; ++e) {
                    int d = d0 + e;
                    int byte_off = d * KVBLK * 2 + ((jp * 4) ^ ((d & 7) << 4));
                    __bf16 pair[2] = {vsta[r][e], vstb[r][e]};
                    *(uint32_t*)((char*)lds.vt[par] + byte_off) = *(uint32_t*)pair;
                }
            }
        }
        if constexpr (!LEAN)
            if (mbase && tid < KVBLK) lds.kmask[par][tid] = mst;
    };

    // 3-deep pipeline over DOUBLE-buffered LDS: one barrier per tile; LDS
    // writes and the next-next tile's HBM loads fully overlap the MFMAs
    const float scale2 = P.scale * LOG2E;    // softmax runs in the exp2 domain
    if (t_lo < t_hi) {
        load_tile();
        write_tile(t_lo & 1);
        if constexpr (LEAN) {
            if (t_lo + 1 < t_hi) load_tile();
        } else {
            if (P.ablate == 1) write_tile((t_lo & 1) ^ 1);   // both buffers valid
            if (t_lo + 1 < t_hi && P.ablate != 1) load_tile();
        }
    }

    for (int t = t_lo; t < t_hi; ++t) {
        const int par = t & 1;
        const long j0 = (long)t * KVBLK;
        const long jmax = min(j0 + KVBLK, P.nk) - 1;
        bool full_tile =
            (jmax - j0 == KVBLK - 1) &&
            M.uncut(wg_q_min, wg_q_max, j0, jmax);
        if constexpr (!LEAN) full_tile = full_tile && !P.kmask && !P.bias;

        __syncthreads();
        bool stamp = false;
        if constexpr (!LEAN)
            stamp = P.ticks && blockIdx.x == 0 && bh == 0 && tid == 0
                    && blockIdx.z == 0;
        FWD_STAMP(0);

        // ---- QK^T: S^T[kv][q] for the NBLK 32-row kv blocks
        f32x16 s[NBLK];
        #pragma unroll
        for (int kb = 0; kb < NBLK; ++kb) s[kb] = f32x16{};
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int kb = 0; kb < NBLK; ++kb) {
            int krow = kb * 32 + l31;
            #pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                int chunk = ks * 2 + lhi;
                bf16x8 kf = *(const bf16x8*)(lds.k[par] + krow * D + swz<D / 8>(krow, chunk) * 8);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kb], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        FWD_STAMP(1);

        // stage tile t+1 into the other buffer while the MFMAs above retire
        bool restage = true;
        if constexpr (!LEAN) restage = P.ablate != 1;
        if (restage) {
            if (t + 1 < t_hi) write_tile(par ^ 1);
            if (t + 2 < t_hi) load_tile();
        }
        FWD_STAMP(2);

        if constexpr (!LEAN) if (P.ablate == 2) {
            // diagnostics: skip softmax VALU, feed PV garbage fragments kept
            // alive via asm (rule 17: a skipped phase must not DCE upstream)
            uint32_t gfrag[4];
            #pragma unroll
            for (int c = 0; c < 4; ++c) {
                union { float f; uint32_t u; } cv; cv.f = s[0][c];
                gfrag[c] = cv.u;
                asm volatile("" :: "v"(gfrag[c]));
            }
            #pragma unroll
            for (int db = 0; db < DBLK; ++db) {
                int drow = db * 32 + l31;
                #pragma unroll
                for (int ks = 0; ks < NBLK * 2; ++ks) {
                    int chunk = ks * 2 + lhi;
                    bf16x8 vf = *(const bf16x8*)(lds.vt[par] + drow * KVBLK + swz<KVBLK / 8>(drow, chunk) * 8);
                    o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        vf, *(const bf16x8*)gfrag, o_acc[db], 0, 0, 0);
                }
            }
            continue;
        }

        // ---- scale (exp2 domain), clamp, mask in place.  The full-tile
        // variant must contain NO per-element conditions: a condition inside
        // the unrolled loop is PREDICATED (cndmask per element, executed on
        // every tile) rather than branched — hoist to one scalar branch.
        float smax = MASK_VALUE_F;
        if (full_tile) {
            if constexpr (!SOFTCLAMP) {
                // exp2+fma fold: fmax runs on RAW scores (scale2 > 0 is
                // monotone); the scale is folded into the exp argument as a
                // single v_fma below — saves one VALU per element
                #pragma unroll
                for (int kb = 0; kb < NBLK; ++kb)
                    #pragma unroll
                    for (int r = 0; r < 16; ++r)
                        smax = fmaxf(smax, s[kb][r]);
                smax *= scale2;
            } else {
                #pragma unroll
                for (int kb = 0; kb < NBLK; ++kb)
                    #pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float xs = s[kb][r] * (P.scale * __builtin_amdgcn_rcpf(P.softclamp_value));
                        float x = P.softclamp_value * fast_tanhf(xs) * LOG2E;
                        s[kb][r] = x;
                        smax = fmaxf(smax, x);
                    }
            }
        } else {
            #pragma unroll
            for (int kb = 0; kb < NBLK; ++kb)
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float x;
                    if constexpr (SOFTCLAMP) {
                        float xs = s[kb][r] * (P.scale * __builtin_amdgcn_rcpf(P.softclamp_value));
                        x = P.softclamp_value * fast_tanhf(xs) * LOG2E;
                    } else {
                        x = s[kb][r] * scale2;
                    }
                    long j = j0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    bool ok = j <= jmax;
                    if constexpr (!LEAN) if (P.bias && ok) {
                        // reference semantics: sim = qk*scale + bias
                        // (natural log), applied after softclamp; our
                        // softmax runs in the exp2 domain
                        const long bi = P.bias_mat
                            ? (((long)b * P.h + h) * P.nq + i_clamped) * P.nk + j
                            : ((long)b * P.h + h) * P.nk + j;
                        x += P.bias[bi] * LOG2E;
                    }
                    ok = M.attends(qpos_i, j, ok);
                    if constexpr (!LEAN)
                        if (P.kmask) ok = ok && lds.kmask[par][j - j0];
                    if (!ok) x = MASK_VALUE_F;
                    s[kb][r] = x;
                    smax = fmaxf(smax, x);
                }
        }
        smax = fmaxf(smax, cross_half(smax));
        FWD_STAMP(3);

        // ---- online softmax update (defer-max THR=0: exact — skip the O
        // rescale whenever the running max did not grow on any lane)
        float m_new = fmaxf(m_run, smax);
        const bool any_growth = !__all(smax <= m_run);
        // all-masked rows: m_new == MASK -> exp2(x - m_new) would be 1 for
        // every masked element (out = mean(V) instead of 0).  Clamping the
        // exp-domain max keeps those exps at 0 while leaving real rows
        // (|scores| << 1e37) untouched.
        const float m_exp = fmaxf(m_new, -1.7e38f);
        // full tiles (no softclamp) kept RAW scores: exp2(fma(s, scale2, -m))
        const float escale = (full_tile && !SOFTCLAMP) ? scale2 : 1.f;
        alignas(16) uint32_t pk[NBLK * 8];                          // packed bf16 pairs
        float partial[NBLK * 8];
        #pragma unroll
        for (int x2 = 0; x2 < NBLK * 8; ++x2) {
            float e0 = __builtin_amdgcn_exp2f(
                __builtin_fmaf(s[x2 >> 3][(2 * x2) & 15], escale, -m_exp));
            float e1 = __builtin_amdgcn_exp2f(
                __builtin_fmaf(s[x2 >> 3][(2 * x2 + 1) & 15], escale, -m_exp));
            partial[x2] = e0 + e1;
            pk[x2] = pack_bf16x2(e0, e1);
        }
        // pairwise tree instead of a 32-deep serial dependency chain
        #pragma unroll
        for (int w = NBLK * 4; w >= 1; w >>= 1)
            #pragma unroll
            for (int x2 = 0; x2 < w; ++x2) partial[x2] += partial[x2 + w];
        float rowsum = partial[0];
        rowsum += cross_half(rowsum);
        if (any_growth) {
            float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run = l_run * alpha + rowsum;
            // LEAN: single-issue multiplies (mul_f32) — written plainly the
            // block is SLP-packed into v_pk_mul_f32, a loss beside MFMAs;
            // same IEEE product per element
            #pragma unroll
            for (int db = 0; db < DBLK; ++db)
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (LEAN) o_acc[db][r] = mul_f32(o_acc[db][r], alpha);
                    else o_acc[db][r] *= alpha;
                }
            m_run = m_new;
        } else {
            l_run += rowsum;
        }

        // ---- PV B-operand fragments: pk[kb*8 + x] holds the exp'd pair for
        // kv rows (pattern):
        //   x=0:(0,1)+4lhi  x=1:(2,3)+4lhi  x=2:(8,9)+4lhi   x=3:(10,11)+4lhi
        //   x=4:(16,17)+4lhi x=5:(18,19)+4lhi x=6:(24,25)+4lhi x=7:(26,27)+4lhi
        // The vt image is staged in this k order (kperm_pair), so
        // pk[4*ks .. 4*ks+3] IS the fragment of k-step ks — no lane exchange.

        FWD_STAMP(4);
        // ---- PV: O^T[d][q] += V^T[d][kv] P^T[kv][q]
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int db = 0; db < DBLK; ++db) {
            int drow = db * 32 + l31;
            #pragma unroll
            for (int ks = 0; ks < NBLK * 2; ++ks) {
                int chunk = ks * 2 + lhi;
                bf16x8 vf = *(const bf16x8*)(lds.vt[par] + drow * KVBLK + swz<KVBLK / 8>(drow, chunk) * 8);
                o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    vf, *(const bf16x8*)(pk + 4 * ks), o_acc[db], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        FWD_STAMP(5);
    }

    // ---- epilogue
    if (!row_valid) FWD_EXIT;

    if (split_mode) {
        // write this split's unnormalized partial (merged by attn_fwd_merge)
        const long part = (long)zsplit * P.b * P.h;
        float* mrow = P.m + (part + (long)b * P.h + h) * P.nq;
        float* lrow = P.l + (part + (long)b * P.h + h) * P.nq;
        if (lhi == 0) { mrow[i] = m_run * LN2; lrow[i] = l_run; }
        float* oa = P.o_acc + (part + (long)b * P.h + h) * D * P.nq;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                oa[(long)d * P.nq + i] = o_acc[db][r];
            }
        FWD_EXIT;
    }

    if (P.is_last) {
        float l_safe = fmaxf(l_run, 1e-38f);
        float inv_l = 1.f / l_safe;
        __bf16* ob = (__bf16*)P.out + ((long)b * P.nq + i) * P.h * D + (long)h * D;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int g = 0; g < 4; ++g) {                            // groups of 4 contiguous d
                __bf16 four[4];
                #pragma unroll
                for (int e = 0; e < 4; ++e)
                    four[e] = (__bf16)(o_acc[db][g * 4 + e] * inv_l);
                int d = db * 32 + 8 * g + 4 * lhi;
                *(uint2*)(ob + d) = *(uint2*)four;
            }
        if (lhi == 0) {
            float* lsep = P.lse + ((long)b * P.h + h) * P.nq;
            lsep[i] = __logf(l_safe) + m_run * LN2;
        }
    } else {
        float* mrow = P.m + ((long)b * P.h + h) * P.nq;
        float* lrow = P.l + ((long)b * P.h + h) * P.nq;
        if (lhi == 0) { mrow[i] = m_run * LN2; lrow[i] = l_run; }
        float* oa = P.o_acc + (((long)b * P.h + h) * D) * P.nq;
        #pragma unroll
        for (int db = 0; db < DBLK; ++db)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                oa[(long)d * P.nq + i] = o_acc[db][r];
            }
    }

#undef FWD_STAMP
