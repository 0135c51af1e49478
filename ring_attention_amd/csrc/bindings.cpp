// PyTorch bindings for the ring_attention_amd CDNA4 kernels.
//
// Thin layer: shape/dtype/contiguity checks + parameter marshalling.  All
// allocation happens in Python; kernels are launched on the current HIP
// stream so they compose with RCCL comm streams and hipGraph capture.

#include <torch/extension.h>
#include <cstdlib>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include "attn_common.h"

namespace ring_attn {

#define CHECK_BF16_CONTIG(t) \
    TORCH_CHECK(t.is_contiguous() && t.scalar_type() == at::kBFloat16, #t " must be contiguous bf16")
#define CHECK_F32_CONTIG(t) \
    TORCH_CHECK(t.is_contiguous() && t.scalar_type() == at::kFloat, #t " must be contiguous fp32")

void attn_fwd(
    at::Tensor q, at::Tensor k, at::Tensor v,
    std::optional<at::Tensor> kmask,
    std::optional<at::Tensor> o_acc,
    std::optional<at::Tensor> m,
    std::optional<at::Tensor> l,
    std::optional<at::Tensor> out,
    std::optional<at::Tensor> lse,
    double scale, bool causal, int64_t diag, int64_t q_stride,
    int64_t win, bool has_win,
    bool softclamp, double softclamp_value,
    bool is_first, bool is_last, int64_t kv_split, int64_t ablate,
    std::optional<at::Tensor> ticks,
    std::optional<at::Tensor> bias, bool bias_mat) {
    CHECK_BF16_CONTIG(q); CHECK_BF16_CONTIG(k); CHECK_BF16_CONTIG(v);
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q/k/v must be (B,N,H,D)");
    const int64_t B = q.size(0), Nq = q.size(1), H = q.size(2), D = q.size(3);
    const int64_t Nk = k.size(1), HK = k.size(2);
    TORCH_CHECK(D == 32 || D == 64 || D == 128,
                "head dim must be 32/64/128 (got ", D, "); arbitrary d <= 128 is "
                "padded at the python layer");
    TORCH_CHECK(H % HK == 0, "q heads must be a multiple of kv heads");
    TORCH_CHECK(k.size(0) == B && v.size(0) == B && v.size(1) == Nk && v.size(2) == HK && v.size(3) == D);

    FwdParams p{};
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr();
    p.kmask = nullptr;
    if (kmask.has_value()) {
        TORCH_CHECK(kmask->is_contiguous() && kmask->scalar_type() == at::kByte, "kmask must be contiguous uint8");
        TORCH_CHECK(kmask->size(0) == B && kmask->size(1) == Nk);
        p.kmask = kmask->data_ptr();
    }
    if (kv_split > 1) {
        TORCH_CHECK(o_acc && m && l, "split launches need partial o/m/l buffers");
        CHECK_F32_CONTIG((*o_acc)); CHECK_F32_CONTIG((*m)); CHECK_F32_CONTIG((*l));
        TORCH_CHECK(kv_split <= 16, "kv_split capped at 16");
        TORCH_CHECK(o_acc->numel() == kv_split * B * H * D * Nq
                    && m->numel() == kv_split * B * H * Nq);
        p.o_acc = o_acc->data_ptr<float>();
        p.m = m->data_ptr<float>();
        p.l = l->data_ptr<float>();
    } else if (!(is_first && is_last)) {
        TORCH_CHECK(o_acc && m && l, "multi-pass launches need o_acc/m/l scratch");
        CHECK_F32_CONTIG((*o_acc)); CHECK_F32_CONTIG((*m)); CHECK_F32_CONTIG((*l));
        TORCH_CHECK(o_acc->numel() == B * H * D * Nq && m->numel() == B * H * Nq);
        p.o_acc = o_acc->data_ptr<float>();
        p.m = m->data_ptr<float>();
        p.l = l->data_ptr<float>();
    }
    if (is_last && kv_split <= 1) {
        TORCH_CHECK(out && lse, "last pass needs out/lse");
        CHECK_BF16_CONTIG((*out)); CHECK_F32_CONTIG((*lse));
        TORCH_CHECK(out->sizes() == q.sizes() && lse->numel() == B * H * Nq);
        p.out = out->data_ptr();
        p.lse = lse->data_ptr<float>();
    }
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.group = (int)(H / HK);
    p.nq = Nq; p.nk = Nk;
    p.scale = (float)scale;
    p.softclamp = softclamp; p.softclamp_value = (float)softclamp_value;
    p.causal = causal; p.diag = diag; p.q_stride = q_stride;
    p.win = win; p.has_win = has_win;
    p.is_first = is_first; p.is_last = is_last;
    p.kv_split = (int)kv_split;
    p.ablate = (int)ablate;
    p.ticks = nullptr;
    if (ticks.has_value()) p.ticks = (unsigned long long*)ticks->data_ptr();
    p.bias = nullptr; p.bias_mat = bias_mat ? 1 : 0;
    if (bias.has_value()) {
        CHECK_F32_CONTIG((*bias));
        TORCH_CHECK(bias->numel() == (bias_mat ? B * H * Nq * Nk : B * H * Nk),
                    "bias must be (B,H,Nk) or (B,H,Nq,Nk) fp32");
        p.bias = bias->data_ptr<float>();
    }
    // causal pairing (uniform per-WG work) whenever the diagonal cuts this
    // kv range and nothing incompatible is on (splits balance differently;
    // windows are already uniform; ticks index per tile)
    p.paired = 0;
    {
        const long T = ceil_div(Nq, ROWS_WG);
        // pairing halves grid.x — only engage when the paired grid (times
        // any grid.z split) still fills the 256 CUs (measured: engaging
        // below that idles half the chip and loses)
        const long z = kv_split > 1 ? kv_split : 1;
        if (causal && !has_win && diag < Nk && !bias.has_value()
            && ((T + 1) / 2) * B * H * z >= 256 && !ticks.has_value()
            && ablate == 0 && !std::getenv("RING_ATTN_NO_PAIR"))
            p.paired = (int)T;
    }

    launch_attn_fwd(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "attn_fwd launch failed");
}

void attn_fwd_merge(
    at::Tensor o_part, at::Tensor m_part, at::Tensor l_part,
    std::optional<at::Tensor> o_acc, std::optional<at::Tensor> m,
    std::optional<at::Tensor> l,
    std::optional<at::Tensor> out, std::optional<at::Tensor> lse,
    int64_t splits, int64_t B, int64_t H, int64_t D, int64_t Nq,
    bool is_first, bool is_last) {
    CHECK_F32_CONTIG(o_part); CHECK_F32_CONTIG(m_part); CHECK_F32_CONTIG(l_part);
    TORCH_CHECK(splits >= 1 && splits <= 16);
    TORCH_CHECK(o_part.numel() == splits * B * H * D * Nq);
    FwdMergeParams p{};
    p.o_part = o_part.data_ptr<float>();
    p.m_part = m_part.data_ptr<float>();
    p.l_part = l_part.data_ptr<float>();
    if (!(is_first && is_last)) {
        TORCH_CHECK(o_acc && m && l, "ring merge needs running o_acc/m/l");
        p.o_acc = o_acc->data_ptr<float>();
        p.m = m->data_ptr<float>();
        p.l = l->data_ptr<float>();
    }
    if (is_last) {
        TORCH_CHECK(out && lse);
        CHECK_BF16_CONTIG((*out)); CHECK_F32_CONTIG((*lse));
        p.out = out->data_ptr();
        p.lse = lse->data_ptr<float>();
    }
    p.splits = (int)splits; p.b = (int)B; p.h = (int)H; p.nq = Nq;
    p.is_first = is_first; p.is_last = is_last;
    launch_attn_fwd_merge(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "attn_fwd_merge launch failed");
}

void attn_bwd(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor dout,
    std::optional<at::Tensor> kmask,
    at::Tensor lse, at::Tensor delta,
    std::optional<at::Tensor> dq, std::optional<at::Tensor> dk,
    std::optional<at::Tensor> dv,
    double scale, bool causal, int64_t diag, int64_t q_stride,
    int64_t win, bool has_win,
    bool softclamp, double softclamp_value, bool accumulate, int64_t split,
    int64_t which,     // 0 = both, 1 = dq only, 2 = dk/dv only
    std::optional<at::Tensor> desc_dq,    // int32 (U,3): tile, t_lo, t_hi
    std::optional<at::Tensor> desc_dkv,
    std::optional<at::Tensor> bias, bool bias_mat,
    // fused epilogue: final-layout bf16 gradients written by the kernels
    // themselves (dq (B,Nq,H,D); dk, dv (B,Nk,HK,D)); single-pass only
    std::optional<at::Tensor> dq_bf, std::optional<at::Tensor> dk_bf,
    std::optional<at::Tensor> dv_bf) {
    CHECK_BF16_CONTIG(q); CHECK_BF16_CONTIG(k); CHECK_BF16_CONTIG(v); CHECK_BF16_CONTIG(dout);
    CHECK_F32_CONTIG(lse); CHECK_F32_CONTIG(delta);
    const int64_t B = q.size(0), Nq = q.size(1), H = q.size(2), D = q.size(3);
    const int64_t Nk = k.size(1), HK = k.size(2);
    TORCH_CHECK(D == 32 || D == 64 || D == 128, "head dim must be 32/64/128");
    TORCH_CHECK(lse.numel() == B * H * Nq && delta.numel() == B * H * Nq);
    const bool run_dq = which == 0 || which == 1;
    const bool run_dkv = which == 0 || which == 2;
    if (dq_bf || dk_bf || dv_bf) {
        // the other modes sum in fp32 across workgroups (grid.z splits,
        // descriptor units) or across hops (accumulate): rounding per
        // contribution would change the result
        TORCH_CHECK(split <= 1 && !accumulate && !desc_dq && !desc_dkv,
                    "bf16 gradient outputs need a single-pass launch "
                    "(split <= 1, no descriptors, accumulate=false)");
        TORCH_CHECK(dk_bf.has_value() == dv_bf.has_value(),
                    "dk_bf and dv_bf go together");
    }
    if (dq_bf) {
        CHECK_BF16_CONTIG((*dq_bf));
        TORCH_CHECK(dq_bf->sizes() == q.sizes(), "dq_bf must be (B,Nq,H,D)");
        TORCH_CHECK((uintptr_t)dq_bf->data_ptr() % 8 == 0, "dq_bf must be 8-byte aligned");
    } else if (run_dq) {
        TORCH_CHECK(dq.has_value(), "dq launch needs an fp32 dq or a bf16 dq_bf");
    }
    if (dk_bf) {
        CHECK_BF16_CONTIG((*dk_bf)); CHECK_BF16_CONTIG((*dv_bf));
        TORCH_CHECK(dk_bf->sizes() == k.sizes() && dv_bf->sizes() == v.sizes(),
                    "dk_bf/dv_bf must be (B,Nk,HK,D)");
        // rows leave the kernel as 16-byte stores
        TORCH_CHECK((uintptr_t)dk_bf->data_ptr() % 16 == 0
                    && (uintptr_t)dv_bf->data_ptr() % 16 == 0,
                    "dk_bf/dv_bf must be 16-byte aligned");
    } else if (run_dkv) {
        TORCH_CHECK(dk.has_value() && dv.has_value(),
                    "dk/dv launch needs fp32 dk, dv or bf16 dk_bf, dv_bf");
    }
    if (dq) { CHECK_F32_CONTIG((*dq)); TORCH_CHECK(dq->numel() == q.numel()); }
    if (dk) { CHECK_F32_CONTIG((*dk)); TORCH_CHECK(dk->numel() == k.numel()); }
    if (dv) { CHECK_F32_CONTIG((*dv)); TORCH_CHECK(dv->numel() == v.numel()); }

    BwdParams p{};
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.dout = dout.data_ptr();
    p.kmask = nullptr;
    if (kmask.has_value()) {
        TORCH_CHECK(kmask->is_contiguous() && kmask->scalar_type() == at::kByte);
        p.kmask = kmask->data_ptr();
    }
    p.lse = lse.data_ptr<float>(); p.delta = delta.data_ptr<float>();
    p.dq = dq ? dq->data_ptr<float>() : nullptr;
    p.dk = dk ? dk->data_ptr<float>() : nullptr;
    p.dv = dv ? dv->data_ptr<float>() : nullptr;
    p.dq_bf = dq_bf ? dq_bf->data_ptr() : nullptr;
    p.dk_bf = dk_bf ? dk_bf->data_ptr() : nullptr;
    p.dv_bf = dv_bf ? dv_bf->data_ptr() : nullptr;
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.group = (int)(H / HK);
    p.nq = Nq; p.nk = Nk;
    p.scale = (float)scale;
    p.softclamp = softclamp; p.softclamp_value = (float)softclamp_value;
    p.causal = causal; p.diag = diag; p.q_stride = q_stride;
    p.win = win; p.has_win = has_win;
    p.accumulate = accumulate;
    p.split = (int)split;
    p.bias = nullptr; p.bias_mat = bias_mat ? 1 : 0;
    if (bias.has_value()) {
        CHECK_F32_CONTIG((*bias));
        TORCH_CHECK(bias->numel() == (bias_mat ? B * H * Nq * Nk : B * H * Nk));
        p.bias = bias->data_ptr<float>();
    }

    // causal pairing: uniform per-WG work when the diagonal cuts this range.
    // dq pairs over Q tiles, dkv over KV tiles (different counts when the
    // kv range is gathered), so set per launch.
    const bool pair_ok = causal && !has_win && diag < Nk
                         && !bias.has_value()
                         && !std::getenv("RING_ATTN_NO_PAIR");
    const long z = split > 1 ? split : 1;
    auto set_desc = [&](const std::optional<at::Tensor>& dsc) {
        p.desc = nullptr; p.n_units = 0;
        if (dsc.has_value()) {
            TORCH_CHECK(dsc->is_contiguous() && dsc->scalar_type() == at::kInt
                        && dsc->dim() == 2 && dsc->size(1) == 3,
                        "desc must be contiguous int32 (U,3)");
            p.desc = dsc->data_ptr<int>();
            p.n_units = dsc->size(0);
        }
    };
    if (run_dq) {
        const long Tq = ceil_div(Nq, ROWS_WG);
        set_desc(desc_dq);
        p.paired = (!p.desc && pair_ok && ((Tq + 1) / 2) * B * H * z >= 256)
                       ? (int)Tq : 0;
        launch_attn_bwd_dq(p, (int)D, at::hip::getCurrentHIPStream());
    }
    if (run_dkv) {
        const long Tk = ceil_div(Nk, ROWS_WG);
        set_desc(desc_dkv);
        p.paired = (!p.desc && pair_ok && ((Tk + 1) / 2) * B * HK * z >= 256)
                       ? (int)Tk : 0;
        launch_attn_bwd_dkv(p, (int)D, at::hip::getCurrentHIPStream());
    }
    TORCH_CHECK(hipGetLastError() == hipSuccess, "attn_bwd launch failed");
}

std::vector<std::optional<at::Tensor>> attn_bwd_finalize(
    std::optional<at::Tensor> dk, std::optional<at::Tensor> dv,
    std::optional<at::Tensor> dq) {
    // dk fp32 (B,HK,Nk,D), dv fp32 (B,HK,D,Nk) -> bf16 (B,Nk,HK,D) each;
    // dq fp32 (any shape, last dim D) -> bf16 same shape.  One launch.
    // Returns (dq_bf, dk_bf, dv_bf); absent inputs give None.
    TORCH_CHECK(dk.has_value() == dv.has_value(), "dk and dv go together");
    TORCH_CHECK(dk || dq, "nothing to finalize");
    BwdFinalizeParams p{};
    std::optional<at::Tensor> dq_bf, dk_bf, dv_bf;
    int64_t D = 0;
    if (dk) {
        CHECK_F32_CONTIG((*dk)); CHECK_F32_CONTIG((*dv));
        TORCH_CHECK(dk->dim() == 4 && dv->dim() == 4, "dk (B,HK,Nk,D), dv (B,HK,D,Nk)");
        const int64_t B = dk->size(0), HK = dk->size(1), Nk = dk->size(2);
        D = dk->size(3);
        TORCH_CHECK(dv->size(0) == B && dv->size(1) == HK && dv->size(2) == D
                    && dv->size(3) == Nk, "dv must be (B,HK,D,Nk)");
        TORCH_CHECK((uintptr_t)dk->data_ptr() % 16 == 0, "dk must be 16-byte aligned");
        dk_bf = at::empty({B, Nk, HK, D}, dk->options().dtype(at::kBFloat16));
        dv_bf = at::empty({B, Nk, HK, D}, dk->options().dtype(at::kBFloat16));
        p.dk = dk->data_ptr<float>(); p.dv = dv->data_ptr<float>();
        p.dk_bf = dk_bf->data_ptr(); p.dv_bf = dv_bf->data_ptr();
        p.b = (int)B; p.hk = (int)HK; p.nk = Nk;
    }
    if (dq) {
        CHECK_F32_CONTIG((*dq));
        TORCH_CHECK(dq->dim() >= 1 && (D == 0 || dq->size(-1) == D),
                    "dq head dim must match dk");
        if (D == 0) D = dq->size(-1);
        TORCH_CHECK((uintptr_t)dq->data_ptr() % 16 == 0, "dq must be 16-byte aligned");
        dq_bf = at::empty_like(*dq, dq->options().dtype(at::kBFloat16));
        p.dq = dq->data_ptr<float>(); p.dq_bf = dq_bf->data_ptr();
        p.dq_elems = dq->numel();
    }
    TORCH_CHECK(D == 32 || D == 64 || D == 128, "head dim must be 32/64/128");
    launch_attn_bwd_finalize(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "attn_bwd_finalize launch failed");
    return {dq_bf, dk_bf, dv_bf};
}

at::Tensor rotary_apply(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t, double sin_sign) {
    // x bf16 (B, N, H, D); cos/sin fp32 (N, D/2)
    CHECK_BF16_CONTIG(x);
    CHECK_F32_CONTIG(cos_t); CHECK_F32_CONTIG(sin_t);
    const int64_t B = x.size(0), N = x.size(1), H = x.size(2), D = x.size(3);
    TORCH_CHECK(D == 32 || D == 64 || D == 128, "head dim must be 32/64/128");
    TORCH_CHECK(cos_t.size(0) == N && cos_t.size(1) == D / 2);
    auto out = at::empty_like(x);
    RotaryParams p{};
    p.x = x.data_ptr();
    p.cos_t = cos_t.data_ptr<float>();
    p.sin_t = sin_t.data_ptr<float>();
    p.out = out.data_ptr();
    p.rows = B * N * H;
    p.n = (int)N; p.h = (int)H; p.d = (int)D;
    p.sin_sign = (float)sin_sign;
    launch_rotary(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "rotary launch failed");
    return out;
}

// What the three decode-partial bindings share: the kv-split S, the fp32
// partials (out (S,B,H,NQ,D), lse (S,B,H,NQ,1)) and the default sm_scale.
// S is chunks_in when forced, else decode_default_chunks on `span`, the
// longest key span of a row (GPU-swept, tools/*decode_sweep*.py: 128k/1M
// bf16: 155/983 -> 112/607 us; fp8: 109/250 -> 60/247 us; GQA 32q/4kv:
// 229 -> 177 us).
struct DecodePartials {
    at::Tensor out, lse;
    int64_t chunks;
    float scale;
};

static DecodePartials decode_partials(const at::Tensor& q, int64_t span,
                                      int64_t chunks_in, double sm_scale) {
    const int64_t B = q.size(0), H = q.size(1), NQ = q.size(2), D = q.size(3);
    const int64_t waves = B * H * NQ;
    DecodePartials r;
    r.chunks = chunks_in > 0 ? chunks_in : decode_default_chunks(span, waves);
    TORCH_CHECK(r.chunks <= 65535, "chunks must fit grid.y");
    TORCH_CHECK((waves + 3) / 4 * r.chunks < (int64_t(1) << 31), "grid too large");
    r.out = at::empty({r.chunks, B, H, NQ, D}, q.options().dtype(at::kFloat));
    r.lse = at::empty({r.chunks, B, H, NQ, 1}, q.options().dtype(at::kFloat));
    r.scale = sm_scale > 0 ? (float)sm_scale : (float)(1.0 / std::sqrt((double)D));
    return r;
}

std::vector<at::Tensor> decode_partial(at::Tensor q, at::Tensor k, at::Tensor v,
                                       double sm_scale, int64_t chunks_in) {
    // q (B,HQ,NQ,D); k,v (B,HK,N,D) bf16 — NQ query tokens (speculative /
    // tree heads), HQ % HK == 0 (GQA, tile pairing qh % hk)
    // -> (out fp32 (S,B,HQ,NQ,D), lse fp32 (S,B,HQ,NQ,1)): S kv-chunk
    //    partials, merged by the caller with the logsumexp combine
    CHECK_BF16_CONTIG(q); CHECK_BF16_CONTIG(k); CHECK_BF16_CONTIG(v);
    const int64_t B = q.size(0), H = q.size(1), NQ = q.size(2), D = q.size(3);
    const int64_t HK = k.size(1), N = k.size(2);
    TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128");
    TORCH_CHECK(H % HK == 0, "q heads must be a multiple of kv heads");
    DecodePartials r = decode_partials(q, N, chunks_in, sm_scale);
    DecodeParams p{};
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr();
    p.out = r.out.data_ptr<float>(); p.lse = r.lse.data_ptr<float>();
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.nq = (int)NQ; p.n = N;
    p.scale = r.scale;
    p.chunks = r.chunks;
    launch_decode_partial(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "decode launch failed");
    return {r.out, r.lse};
}

std::vector<at::Tensor> attn_fwd_fp8(at::Tensor q8, at::Tensor k8, at::Tensor v8t,
                                      at::Tensor qs, at::Tensor ks, at::Tensor vs,
                                      double sm_scale, bool causal, int64_t nk_true,
                                      int64_t diag, int64_t q_stride, bool has_win,
                                      int64_t win) {
    // MX-FP8 serving forward (see attn_fwd_fp8.hip header for scope); the
    // mask is attn_mask.h's: causal at qpos(i) = i * q_stride + diag, window
    // qpos(i) - j <= win when has_win (the defaults are the standard mask):
    //   q8 (B,Nq,H,D) u8 e4m3; k8 (B,Nk,H,D) u8; v8t (B,H,D,Nk) u8
    //   qs (B,Nq,H) u8 e8m0(+127); ks (B,Nk,H) u8; vs (B,H,D,Nk/64) u8
    // -> out bf16 (B,Nq,H,D), lse fp32 (B,H,Nq)
    for (auto* t : {&q8, &k8, &v8t, &qs, &ks, &vs}) {
        TORCH_CHECK(t->scalar_type() == at::kByte && t->is_contiguous(),
                    "fp8 operands must be contiguous uint8 views");
    }
    const int64_t B = q8.size(0), NQ = q8.size(1), H = q8.size(2), D = q8.size(3);
    const int64_t NK = k8.size(1), HK = k8.size(2);
    TORCH_CHECK(D == 64 || D == 128, "fp8 path: head dim 64 or 128");
    TORCH_CHECK(H % HK == 0, "fp8 path: q heads must be a multiple of kv heads");
    TORCH_CHECK(NQ % 256 == 0, "fp8 path: nq must be a multiple of 256 (v0)");
    TORCH_CHECK(NK % 128 == 0, "fp8 path: nk must be a multiple of 128 (v0)");
    TORCH_CHECK(q_stride >= 1, "fp8 path: q_stride must be >= 1");
    if (nk_true <= 0) nk_true = NK;
    TORCH_CHECK(v8t.size(1) == HK && v8t.size(3) == NK && v8t.size(2) == D
                && vs.size(1) == HK && vs.size(3) == NK / 64);
    TORCH_CHECK(qs.numel() == B * NQ * H * (D / 64)
                && ks.numel() == B * NK * HK * (D / 64),
                "q/k scales must be per (row, 64-d chunk)");
    auto out = at::empty({B, NQ, H, D}, q8.options().dtype(at::kBFloat16));
    auto lse = at::empty({B, H, NQ}, q8.options().dtype(at::kFloat));
    Fp8FwdParams p{};
    p.q = q8.data_ptr(); p.k = k8.data_ptr(); p.vt = v8t.data_ptr();
    p.qs = qs.data_ptr(); p.ks = ks.data_ptr(); p.vs = vs.data_ptr();
    p.out = out.data_ptr(); p.lse = lse.data_ptr<float>();
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.nq = NQ; p.nk = NK;
    p.nk_true = nk_true;
    p.nvs = (int)(NK / 64);
    p.causal = causal ? 1 : 0;
    p.has_win = has_win ? 1 : 0;
    p.diag = diag; p.q_stride = q_stride; p.win = has_win ? win : 0;
    p.scale = sm_scale > 0 ? (float)sm_scale : (float)(1.0 / std::sqrt((double)D));
    launch_attn_fwd_fp8(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "attn_fwd_fp8 launch failed");
    return {out, lse};
}

std::vector<at::Tensor> decode_partial_fp8(at::Tensor q, at::Tensor k8, at::Tensor v8,
                                           at::Tensor ks, at::Tensor vs,
                                           double sm_scale, int64_t chunks_in) {
    // FP8 KV-cache decode partial: q bf16 (B,HQ,NQ,D); k8/v8 e4m3 u8
    // (B,HK,N,D) with per-row e8m0 scales ks/vs (B,HK,N).  Same output
    // contract as decode_partial: (out fp32 (S,B,HQ,NQ,D), lse (S,B,HQ,NQ,1)).
    CHECK_BF16_CONTIG(q);
    for (auto* t : {&k8, &v8, &ks, &vs})
        TORCH_CHECK(t->scalar_type() == at::kByte && t->is_contiguous(),
                    "fp8 cache operands must be contiguous uint8");
    const int64_t B = q.size(0), H = q.size(1), NQ = q.size(2), D = q.size(3);
    const int64_t HK = k8.size(1), N = k8.size(2);
    TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128");
    TORCH_CHECK(H % HK == 0, "q heads must be a multiple of kv heads");
    TORCH_CHECK(ks.numel() == B * HK * N && vs.numel() == B * HK * N);
    DecodePartials r = decode_partials(q, N, chunks_in, sm_scale);
    DecodeParams p{};
    p.q = q.data_ptr(); p.k = k8.data_ptr(); p.v = v8.data_ptr();
    p.kscale = ks.data_ptr(); p.vscale = vs.data_ptr();
    p.out = r.out.data_ptr<float>(); p.lse = r.lse.data_ptr<float>();
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.nq = (int)NQ; p.n = N;
    p.scale = r.scale;
    p.chunks = r.chunks;
    launch_decode_partial_fp8(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "decode fp8 launch failed");
    return {r.out, r.lse};
}

std::vector<at::Tensor> decode_merge(at::Tensor outs, at::Tensor lses) {
    // fuse the S kv-chunk partial merge: outs (S,B,H,NQ,D) fp32,
    // lses (S,B,H,NQ,1) fp32 -> (out (B,H,NQ,D) fp32, lse (B,H,NQ,1) fp32)
    CHECK_F32_CONTIG(outs); CHECK_F32_CONTIG(lses);
    const int64_t S = outs.size(0), B = outs.size(1), H = outs.size(2),
                  NQ = outs.size(3), D = outs.size(4);
    TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128");
    auto out = at::empty({B, H, NQ, D}, outs.options());
    auto lse = at::empty({B, H, NQ, 1}, outs.options());
    DecodeMergeParams p{};
    p.outs = outs.data_ptr<float>(); p.lses = lses.data_ptr<float>();
    p.out = out.data_ptr<float>(); p.lse = lse.data_ptr<float>();
    p.rows = B * H * NQ; p.s = (int)S;
    launch_decode_merge(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "decode merge launch failed");
    return {out, lse};
}

// shared checks of the paged-cache operands; returns log2(page_size)
static int check_paged_pool(const at::Tensor& ref, const at::Tensor& k_pages,
                            const at::Tensor& v_pages,
                            const std::optional<at::Tensor>& k_scales,
                            const std::optional<at::Tensor>& v_scales,
                            const at::Tensor& block_table, const at::Tensor& seq_lens,
                            int64_t B, int64_t D, bool* fp8_out) {
    TORCH_CHECK(k_pages.dim() == 4 && v_pages.dim() == 4,
                "k_pages/v_pages must be (num_pages, HK, page_size, D)");
    TORCH_CHECK(k_pages.is_contiguous() && v_pages.is_contiguous(),
                "k_pages/v_pages must be contiguous");
    TORCH_CHECK(k_pages.sizes() == v_pages.sizes()
                && k_pages.scalar_type() == v_pages.scalar_type(),
                "k_pages and v_pages must match in shape and dtype (dv == d)");
    const bool fp8 = k_pages.scalar_type() == at::kByte;
    TORCH_CHECK(fp8 || k_pages.scalar_type() == at::kBFloat16,
                "pages must be bf16 or uint8 (e4m3 bytes)");
    const int64_t P = k_pages.size(0), HK = k_pages.size(1), PS = k_pages.size(2);
    TORCH_CHECK(k_pages.size(3) == D, "page head dim must equal q/k_new head dim");
    TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128");
    TORCH_CHECK(PS >= 16 && PS <= 256 && (PS & (PS - 1)) == 0,
                "page_size must be a power of two in [16, 256] (got ", PS, ")");
    TORCH_CHECK(P < (int64_t(1) << 31), "too many pages");
    if (fp8) {
        TORCH_CHECK(k_scales.has_value() && v_scales.has_value(),
                    "fp8 pages need k_scales/v_scales");
        for (auto* t : {&*k_scales, &*v_scales})
            TORCH_CHECK(t->scalar_type() == at::kByte && t->is_contiguous()
                        && t->device() == k_pages.device()
                        && t->dim() == 3 && t->size(0) == P && t->size(1) == HK
                        && t->size(2) == PS,
                        "scales must be contiguous uint8 (num_pages, HK, page_size)");
    }
    TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.is_contiguous()
                && block_table.dim() == 2 && block_table.size(0) == B,
                "block_table must be contiguous int32 (B, max_pages_per_seq)");
    TORCH_CHECK(seq_lens.scalar_type() == at::kInt && seq_lens.is_contiguous()
                && seq_lens.dim() == 1 && seq_lens.size(0) == B,
                "seq_lens must be contiguous int32 (B,)");
    TORCH_CHECK(block_table.device() == ref.device() && seq_lens.device() == ref.device()
                && k_pages.device() == ref.device() && v_pages.device() == ref.device(),
                "pages, block_table and seq_lens must be on the same device as q/k_new");
    TORCH_CHECK(block_table.size(1) * PS < (int64_t(1) << 31), "table too wide");
    *fp8_out = fp8;
    int shift = 0;
    while ((int64_t(1) << shift) < PS) ++shift;
    return shift;
}

std::vector<at::Tensor> decode_partial_paged(
    at::Tensor q, at::Tensor k_pages, at::Tensor v_pages,
    std::optional<at::Tensor> k_scales, std::optional<at::Tensor> v_scales,
    at::Tensor block_table, at::Tensor seq_lens, int64_t max_seq_len,
    double sm_scale, bool causal, int64_t chunks_in,
    bool has_win, int64_t win, std::optional<at::Tensor> kv_after) {
    // q bf16 (B,HQ,NQ,D); pages (P,HK,PS,D) bf16, or uint8 e4m3 with per-row
    // e8m0 scales (P,HK,PS) — the page dtype selects the fp8 kernel;
    // block_table int32 (B,max_pages), seq_lens int32 (B,).  max_seq_len is
    // the HOST's upper bound of seq_lens (drives the kv-split; no device
    // read).  Same output contract as decode_partial.  has_win / win: the
    // token-exact lookback window; kv_after int32 (B,) = tokens of each
    // sequence held by later ranks (None = 0).
    CHECK_BF16_CONTIG(q);
    TORCH_CHECK(q.dim() == 4, "q must be (B,HQ,NQ,D)");
    const int64_t B = q.size(0), H = q.size(1), NQ = q.size(2), D = q.size(3);
    bool fp8 = false;
    const int shift = check_paged_pool(q, k_pages, v_pages, k_scales, v_scales,
                                       block_table, seq_lens, B, D, &fp8);
    const int64_t HK = k_pages.size(1);
    TORCH_CHECK(H % HK == 0, "q heads must be a multiple of kv heads");
    TORCH_CHECK(max_seq_len >= 0
                && max_seq_len <= block_table.size(1) * k_pages.size(2),
                "max_seq_len exceeds what block_table can address");
    TORCH_CHECK(!has_win || (win >= 0 && win < (int64_t(1) << 40)),
                "win must lie in [0, 2^40)");
    if (has_win && kv_after.has_value()) {
        TORCH_CHECK(kv_after->scalar_type() == at::kInt && kv_after->is_contiguous()
                    && kv_after->dim() == 1 && kv_after->size(0) == B
                    && kv_after->device() == q.device(),
                    "kv_after must be contiguous int32 (B,) on q's device");
    }
    // the kv-split follows the longest sequence, or with a window the
    // longest row span (launch_decode_partial_paged)
    const int64_t span = has_win ? std::min<int64_t>(max_seq_len, win + NQ + 63)
                                 : max_seq_len;
    DecodePartials r = decode_partials(q, span, chunks_in, sm_scale);
    if (B * H * NQ == 0) return {r.out, r.lse};
    PagedDecodeParams p{};
    p.q = q.data_ptr();
    p.k_pages = k_pages.data_ptr(); p.v_pages = v_pages.data_ptr();
    if (fp8) { p.kscale = k_scales->data_ptr(); p.vscale = v_scales->data_ptr(); }
    p.block_table = block_table.data_ptr<int>();
    p.seq_lens = seq_lens.data_ptr<int>();
    p.out = r.out.data_ptr<float>(); p.lse = r.lse.data_ptr<float>();
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.nq = (int)NQ;
    p.page_shift = shift;
    p.max_pages = (int)block_table.size(1);
    p.num_pages = (int)k_pages.size(0);
    p.causal = causal ? 1 : 0;
    // workgroup order: a batch can be ragged, so its kv chunks are the fast
    // workgroup index (every sequence spreads over all XCDs: ragged b=8
    // 1k..128k 601 -> 241 us); a single sequence keeps the dense kernels'
    // order, which measured at dense speed for every page size / table.
    // RING_ATTN_PAGED_ORDER=row|chunk forces either (A/B).
    const char* order = std::getenv("RING_ATTN_PAGED_ORDER");
    p.chunk_major = order && order[0] == 'r' ? 0
                  : order && order[0] == 'c' ? 1 : (B > 1 ? 1 : 0);
    p.scale = r.scale;
    p.chunks = r.chunks;
    p.max_seq_len = max_seq_len;
    p.has_win = has_win ? 1 : 0;
    p.win = has_win ? win : 0;
    p.kv_after = has_win && kv_after.has_value() ? kv_after->data_ptr<int>() : nullptr;
    launch_decode_partial_paged(p, (int)D, fp8, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "paged decode launch failed");
    return {r.out, r.lse};
}

void paged_kv_append(
    at::Tensor k_new, at::Tensor v_new, at::Tensor k_pages, at::Tensor v_pages,
    std::optional<at::Tensor> k_scales, std::optional<at::Tensor> v_scales,
    at::Tensor block_table, at::Tensor seq_lens, at::Tensor append_lens) {
    // k_new/v_new bf16 (B,HK,T,D): token t < append_lens[b] of sequence b is
    // written at position seq_lens[b] + t (seq_lens = lengths BEFORE the
    // append; the caller advances them).  uint8 pages quantise in flight.
    CHECK_BF16_CONTIG(k_new); CHECK_BF16_CONTIG(v_new);
    TORCH_CHECK(k_new.dim() == 4 && k_new.sizes() == v_new.sizes(),
                "k_new/v_new must both be (B,HK,T,D)");
    const int64_t B = k_new.size(0), HK = k_new.size(1), T = k_new.size(2), D = k_new.size(3);
    bool fp8 = false;
    const int shift = check_paged_pool(k_new, k_pages, v_pages, k_scales, v_scales,
                                       block_table, seq_lens, B, D, &fp8);
    TORCH_CHECK(k_pages.size(1) == HK, "kv heads of k_new and the pages differ");
    TORCH_CHECK(append_lens.scalar_type() == at::kInt && append_lens.is_contiguous()
                && append_lens.dim() == 1 && append_lens.size(0) == B
                && append_lens.device() == k_new.device(),
                "append_lens must be contiguous int32 (B,) on the same device");
    TORCH_CHECK(B * HK * T < (int64_t(1) << 33), "append too large");
    PagedAppendParams p{};
    p.k_new = k_new.data_ptr(); p.v_new = v_new.data_ptr();
    p.k_pages = k_pages.data_ptr(); p.v_pages = v_pages.data_ptr();
    if (fp8) { p.kscale = k_scales->data_ptr(); p.vscale = v_scales->data_ptr(); }
    p.block_table = block_table.data_ptr<int>();
    p.seq_lens = seq_lens.data_ptr<int>();
    p.append_lens = append_lens.data_ptr<int>();
    p.b = (int)B; p.hk = (int)HK; p.t = (int)T;
    p.page_shift = shift;
    p.max_pages = (int)block_table.size(1);
    p.num_pages = (int)k_pages.size(0);
    launch_paged_kv_append(p, (int)D, fp8, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "paged append launch failed");
}

void attn_fwd_paged(
    at::Tensor q, at::Tensor k_pages, at::Tensor v_pages,
    std::optional<at::Tensor> k_scales, std::optional<at::Tensor> v_scales,
    at::Tensor block_table, at::Tensor seq_lens, at::Tensor q_lens,
    std::optional<at::Tensor> out, std::optional<at::Tensor> lse,
    std::optional<at::Tensor> o_part, std::optional<at::Tensor> m_part,
    std::optional<at::Tensor> l_part,
    double scale, bool causal, int64_t win, bool has_win, int64_t kv_split) {
    // q bf16 (B,T,H,D); pool operands as decode_partial_paged; q_lens int32
    // (B,).  kv_split <= 1 writes out bf16 (B,T,H,D) + lse fp32 (B,H,T);
    // kv_split > 1 writes the (S,B,H,D,T) + m,l partials for attn_fwd_merge.
    CHECK_BF16_CONTIG(q);
    TORCH_CHECK(q.dim() == 4, "q must be (B,T,H,D)");
    const int64_t B = q.size(0), T = q.size(1), H = q.size(2), D = q.size(3);
    bool fp8 = false;
    const int shift = check_paged_pool(q, k_pages, v_pages, k_scales, v_scales,
                                       block_table, seq_lens, B, D, &fp8);
    const int64_t HK = k_pages.size(1);
    TORCH_CHECK(H % HK == 0, "q heads must be a multiple of kv heads");
    TORCH_CHECK(q_lens.scalar_type() == at::kInt && q_lens.is_contiguous()
                && q_lens.dim() == 1 && q_lens.size(0) == B
                && q_lens.device() == q.device(),
                "q_lens must be contiguous int32 (B,) on the same device");
    TORCH_CHECK(B * H <= 65535, "B*H must fit grid.y");
    TORCH_CHECK(T < (int64_t(1) << 31), "T too large");
    TORCH_CHECK(!has_win || win >= 0, "window must be >= 0");
    PagedPrefillParams p{};
    if (kv_split > 1) {
        TORCH_CHECK(kv_split <= 16, "kv_split capped at 16");
        TORCH_CHECK(o_part && m_part && l_part, "split launches need partial o/m/l buffers");
        CHECK_F32_CONTIG((*o_part)); CHECK_F32_CONTIG((*m_part)); CHECK_F32_CONTIG((*l_part));
        TORCH_CHECK(o_part->numel() == kv_split * B * H * D * T
                    && m_part->numel() == kv_split * B * H * T
                    && l_part->numel() == kv_split * B * H * T,
                    "partials must be (S,B,H,D,T) and (S,B,H,T)");
        p.o_part = o_part->data_ptr<float>();
        p.m_part = m_part->data_ptr<float>();
        p.l_part = l_part->data_ptr<float>();
    } else {
        TORCH_CHECK(out && lse, "unsplit launches need out/lse");
        CHECK_BF16_CONTIG((*out)); CHECK_F32_CONTIG((*lse));
        TORCH_CHECK(out->sizes() == q.sizes() && lse->numel() == B * H * T);
        p.out = out->data_ptr();
        p.lse = lse->data_ptr<float>();
    }
    if (B * T * H == 0) return;
    p.q = q.data_ptr();
    p.k_pages = k_pages.data_ptr(); p.v_pages = v_pages.data_ptr();
    if (fp8) { p.kscale = k_scales->data_ptr(); p.vscale = v_scales->data_ptr(); }
    p.block_table = block_table.data_ptr<int>();
    p.seq_lens = seq_lens.data_ptr<int>();
    p.q_lens = q_lens.data_ptr<int>();
    p.b = (int)B; p.h = (int)H; p.hk = (int)HK; p.t = (int)T;
    p.page_shift = shift;
    p.max_pages = (int)block_table.size(1);
    p.num_pages = (int)k_pages.size(0);
    p.causal = causal ? 1 : 0; p.has_win = has_win ? 1 : 0; p.win = win;
    p.scale = (float)scale;
    p.kv_split = (int)kv_split;
    launch_attn_fwd_paged(p, (int)D, fp8, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "paged prefill launch failed");
}

at::Tensor attn_delta(at::Tensor dout, at::Tensor out) {
    // dout, out (B,N,H,D) bf16 -> delta fp32 (B,H,N) = rowsum(dout*out)
    CHECK_BF16_CONTIG(dout); CHECK_BF16_CONTIG(out);
    const int64_t B = dout.size(0), N = dout.size(1), H = dout.size(2), D = dout.size(3);
    TORCH_CHECK(D == 32 || D == 64 || D == 128, "head dim must be 32/64/128");
    auto delta = at::empty({B, H, N}, dout.options().dtype(at::kFloat));
    DeltaParams p{};
    p.dout = dout.data_ptr(); p.out = out.data_ptr();
    p.delta = delta.data_ptr<float>();
    p.rows = B * N * H; p.n = N; p.h = (int)H;
    launch_attn_delta(p, (int)D, at::hip::getCurrentHIPStream());
    TORCH_CHECK(hipGetLastError() == hipSuccess, "delta launch failed");
    return delta;
}

}  // namespace ring_attn

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
    mod.def("attn_fwd", &ring_attn::attn_fwd, "CDNA4 flash attention forward (resumable)",
            py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kmask"),
            py::arg("o_acc"), py::arg("m"), py::arg("l"), py::arg("out"),
            py::arg("lse"), py::arg("scale"), py::arg("causal"), py::arg("diag"),
            py::arg("q_stride"), py::arg("win"), py::arg("has_win"),
            py::arg("softclamp"), py::arg("softclamp_value"), py::arg("is_first"),
            py::arg("is_last"), py::arg("kv_split"), py::arg("ablate"),
            py::arg("ticks"), py::arg("bias") = std::nullopt,
            py::arg("bias_mat") = false);
    mod.def("attn_fwd_merge", &ring_attn::attn_fwd_merge, "merge kv-split partials");
    mod.def("attn_bwd", &ring_attn::attn_bwd, "CDNA4 flash attention backward",
            py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dout"),
            py::arg("kmask"), py::arg("lse"), py::arg("delta"), py::arg("dq"),
            py::arg("dk"), py::arg("dv"), py::arg("scale"), py::arg("causal"),
            py::arg("diag"), py::arg("q_stride"), py::arg("win"),
            py::arg("has_win"), py::arg("softclamp"), py::arg("softclamp_value"),
            py::arg("accumulate"), py::arg("split"), py::arg("which"),
            py::arg("desc_dq"), py::arg("desc_dkv"),
            py::arg("bias") = std::nullopt, py::arg("bias_mat") = false,
            py::arg("dq_bf") = std::nullopt, py::arg("dk_bf") = std::nullopt,
            py::arg("dv_bf") = std::nullopt);
    mod.def("attn_bwd_finalize", &ring_attn::attn_bwd_finalize,
            "fp32 scratch gradients -> final-layout bf16 (one launch)",
            py::arg("dk"), py::arg("dv"), py::arg("dq") = std::nullopt);
    mod.def("decode_partial", &ring_attn::decode_partial, "CDNA4 single-query decode partial",
            py::arg("q"), py::arg("k"), py::arg("v"), py::arg("sm_scale") = -1.0,
            py::arg("chunks") = 0);
    mod.def("attn_fwd_fp8", &ring_attn::attn_fwd_fp8,
            "CDNA4 MX-FP8 serving forward (e4m3 + e8m0 row scales)",
            py::arg("q8"), py::arg("k8"), py::arg("v8t"), py::arg("qs"),
            py::arg("ks"), py::arg("vs"), py::arg("sm_scale") = -1.0,
            py::arg("causal") = false, py::arg("nk_true") = 0,
            py::arg("diag") = 0, py::arg("q_stride") = 1,
            py::arg("has_win") = false, py::arg("win") = 0);
    mod.def("decode_partial_fp8", &ring_attn::decode_partial_fp8,
            "CDNA4 FP8 KV-cache decode partial",
            py::arg("q"), py::arg("k8"), py::arg("v8"), py::arg("ks"),
            py::arg("vs"), py::arg("sm_scale") = -1.0, py::arg("chunks") = 0);
    mod.def("decode_merge", &ring_attn::decode_merge,
            "fused kv-chunk partial merge for decode");
    mod.def("decode_partial_paged", &ring_attn::decode_partial_paged,
            "CDNA4 paged KV-cache decode partial (bf16 or fp8 pages)",
            py::arg("q"), py::arg("k_pages"), py::arg("v_pages"),
            py::arg("k_scales"), py::arg("v_scales"), py::arg("block_table"),
            py::arg("seq_lens"), py::arg("max_seq_len"),
            py::arg("sm_scale") = -1.0, py::arg("causal") = false,
            py::arg("chunks") = 0, py::arg("has_win") = false,
            py::arg("win") = 0, py::arg("kv_after") = py::none());
    mod.def("paged_kv_append", &ring_attn::paged_kv_append,
            "write new tokens into a paged KV cache (fused fp8 quantisation)",
            py::arg("k_new"), py::arg("v_new"), py::arg("k_pages"),
            py::arg("v_pages"), py::arg("k_scales"), py::arg("v_scales"),
            py::arg("block_table"), py::arg("seq_lens"), py::arg("append_lens"));
    mod.def("attn_fwd_paged", &ring_attn::attn_fwd_paged,
            "CDNA4 paged prefill attention (bf16 or fp8 pages, per-sequence lengths)",
            py::arg("q"), py::arg("k_pages"), py::arg("v_pages"),
            py::arg("k_scales"), py::arg("v_scales"), py::arg("block_table"),
            py::arg("seq_lens"), py::arg("q_lens"), py::arg("out"), py::arg("lse"),
            py::arg("o_part"), py::arg("m_part"), py::arg("l_part"),
            py::arg("scale"), py::arg("causal"), py::arg("win"),
            py::arg("has_win"), py::arg("kv_split"));
    // host access to attn_mask.h, the kernels' own mask geometry (no GPU
    // needed): the descriptor builder takes its shapes and bounds from here,
    // and the CPU tests hold it to a brute-force mask
    using ring_attn::Mask;
    using ring_attn::TileRange;
    auto pair = [](TileRange r) { return std::make_pair(r.lo, r.hi); };
    py::class_<Mask>(mod, "Mask", "mask geometry (csrc/attn_mask.h)")
        .def(py::init([](bool causal, long diag, long q_stride, bool has_win, long win) {
                 TORCH_CHECK(q_stride >= 1, "q_stride must be >= 1");
                 return Mask{causal, has_win, diag, q_stride, win};
             }), py::arg("causal"), py::arg("diag") = 0, py::arg("q_stride") = 1,
             py::arg("has_win") = false, py::arg("win") = 0)
        .def("qpos", &Mask::qpos)
        .def("attends", &Mask::attends, py::arg("qpos"), py::arg("j"), py::arg("ok") = true)
        .def("attends_matrix", [](const Mask& m, int64_t nq, int64_t nk) {
                 auto a = at::empty({nq, nk}, at::kBool);   // [i][j] = attends(qpos(i), j)
                 for (int64_t i = 0; i < nq; ++i)
                     for (int64_t j = 0; j < nk; ++j)
                         a.data_ptr<bool>()[i * nk + j] = m.attends(m.qpos(i), j);
                 return a;
             })
        .def("row_cut", [](const Mask& m, long qp, long j0, int w, long nk) {
                 auto r = m.row_cut(qp, j0, w, nk);
                 return std::make_pair(r.lo, r.hi); },
             py::arg("qpos"), py::arg("j0"), py::arg("w"), py::arg("nk"))
        .def("uncut", &Mask::uncut, py::arg("q_lo"), py::arg("q_hi"), py::arg("j0"), py::arg("jmax"))
        .def("kv_tile_range", [pair](const Mask& m, long i_min, long i_max, long nk, int w) {
                 return pair(m.kv_tile_range(i_min, i_max, nk, w)); })
        .def("q_tile_range", [pair](const Mask& m, long j0, long jmax, long nq, int w) {
                 return pair(m.q_tile_range(j0, jmax, nq, w)); });
    mod.def("mask_split_share", [pair](int lo, int hi, int splits, int z) {
        return pair(ring_attn::split_share({lo, hi}, splits, z)); });
    mod.def("mask_tile_shapes", [](int d) {   // tile shapes at head dim d
        return py::dict(py::arg("rows_wg") = ring_attn::ROWS_WG,
                        py::arg("kvblk") = ring_attn::kvblk(d),
                        py::arg("dkv_qt") = ring_attn::DKV_QT,
                        py::arg("fp8_kvblk") = ring_attn::FP8_KVBLK);
    });
    mod.def("attn_delta", &ring_attn::attn_delta, "fused delta = rowsum(dO*O) preprocess");
    mod.def("rotary_apply", &ring_attn::rotary_apply, "fused rotary embedding (table-driven)");
}
