// Conv-net executor (VAE encoder / decoder, HiFi-GAN generator): a loaded op list run over buffers carved from the caller's workspace,
// vb_net_load's validation, and the entry points that run a net.
#include "engine.h"

static size_t net_ws_bytes(const NetProgram& n, int B, int T, std::vector<size_t>* offs) {
    size_t off = 0;
    if (offs) offs->clear();
    for (const vb_buf_desc& d : n.bufs) {
        size_t tl = (size_t)T * d.tmul;
        // (floats per clip; square 3 = two bf16 planes with halo rows, 4 = one: half as many floats, channels % 16 == 0)
        size_t el = d.square == 1 ? tl * tl : (d.square == 2 ? (size_t)d.channels * ((tl + 31) / 32 * 32)
                                  : (d.square == 3 ? (size_t)d.channels * (tl + XT_HEAD + XT_TAIL)
                                  : (d.square == 4 ? ((size_t)d.channels * (tl + XT_HEAD + XT_TAIL) + 1) / 2 : (size_t)d.channels * tl)));
        if (offs) offs->push_back(off);
        off = align_up(off + el * B * sizeof(float));
    }
    return off;
}
// nl (vb_hifigan_forward_lens / vb_vae_decode_lens / vb_vae_encode_lens, after net_lens_check): `in` is the masked copy of the input, every op that writes an
// activation buffer is followed by launch_tail_zero on it, and the fused pairs end row b's intermediate at its own length.  The VAE decoder's
// ops that a zero tail does not settle read the device table: GroupNorm statistics run over the row's own samples, every GroupNorm (+ swish)
// consumer ends the ACTIVATED tensor at the row's own length, the attention softmax runs over the row's own keys.  Null: the plain run,
// nothing added.
int net_run(vb_ctx* ctx, int which, const float* in, int B, int T, float* out, void* ws, hipStream_t st, const NetLens* nl) {
    NetProgram& n = ctx->nets[which];
    if (!n.loaded) VB_FAIL(VB_E_STATE, "net %d not loaded", which);
    VB_HIP(hipSetDevice(ctx->device));
    std::vector<size_t> offs;
    net_ws_bytes(n, B, T, &offs);
    auto ptr = [&](int id) -> float* {
        if (id == VB_BUF_INPUT) return const_cast<float*>(in);
        if (id == VB_BUF_OUTPUT) return out;
        if (id < 0) return nullptr;
        return reinterpret_cast<float*>(static_cast<char*>(ws) + offs[id]);
    };
    auto tlen = [&](int id) -> int {
        if (id == VB_BUF_INPUT) return T * n.in_tmul;
        if (id == VB_BUF_OUTPUT) return T * n.out_tmul;
        return T * n.bufs[id].tmul;
    };
    auto chans = [&](int id) -> int {
        if (id == VB_BUF_INPUT) return n.in_ch;
        if (id == VB_BUF_OUTPUT) return n.out_ch;
        return n.bufs[id].channels;
    };
    auto tmul = [&](int id) -> int { return id == VB_BUF_INPUT ? n.in_tmul : (id == VB_BUF_OUTPUT ? n.out_tmul : n.bufs[id].tmul); };
    auto bstride = [&](int id) -> int64_t {
        if (id >= 0 && n.bufs[id].square == 1) return (int64_t)tlen(id) * tlen(id);
        return (int64_t)chans(id) * tlen(id);
    };
    for (size_t oi = 0; oi < n.ops.size(); ++oi) {
        const vb_net_op& o = n.ops[oi];
        if (o.kind == VB_OP_GN_STATS) {
            float* stp = ptr(o.stats);
            VB_TRY(launch_gn_stats(ptr(o.x), B, o.Ci, tlen(o.x), o.gn_groups, 1e-6f, stp, stp + (size_t)B * o.gn_groups, st, nl ? nl->table : nullptr,
                                   tmul(o.x)));
        } else if (o.kind == VB_OP_SOFTMAX_T) {
            // (lengths: the whole transposed square is written, zeros outside the row's own block - it needs no tail pass)
            VB_TRY(launch_softmax_rows_t(ptr(o.x), B, tlen(o.x), tlen(o.x), ptr(o.out), st, nl ? nl->table : nullptr, tmul(o.x)));
        } else if (o.kind == VB_OP_CONV) {
            ConvArgs a;
            a.x = ptr(o.x); a.x_bstride = bstride(o.x); a.T_in = tlen(o.x);
            if (o.x_planes) {
                // input written by VB_OP_XT_PLANES: its buffer's time length is the (upsampled) length the planes were made for
                a.xt = reinterpret_cast<const bf16_t*>(ptr(o.x));
                a.xt_np = n.bufs[o.x].square == 4 ? 1 : 2;       // (vb_net_load checked the buffer against the weight format)
                a.T_in = o.upsample2 ? tlen(o.x) / 2 : tlen(o.x);
            }
            a.Ci = o.Ci > 0 ? o.Ci : tlen(o.x);            // dynamic channel counts: the VAE attention contracts over T
            a.bias = o.bias; a.Co = o.Co > 0 ? o.Co : tlen(o.out); a.ksize = o.ksize; a.dil = o.dil; a.pad = o.pad; a.upsample2 = o.upsample2;
            a.in_stride = o.in_stride > 1 ? o.in_stride : 1; a.in_phase = o.in_phase;
            a.in_act = o.in_act; a.in_slope = o.in_slope;
            if (o.stats >= 0) {
                float* stp = ptr(o.stats);
                a.gn_mean = stp; a.gn_rstd = stp + (size_t)B * o.gn_groups; a.gn_gamma = o.gn_gamma; a.gn_beta = o.gn_beta;
                a.gn_groups = o.gn_groups;
            }
            // lengths: GroupNorm maps a zero tail to something else, so the window's zero padding starts at the row's own end
            if (nl && (o.in_act == ACT_GN || o.in_act == ACT_GN_SWISH)) { a.row_len = nl->table; a.len_mul = tmul(o.x) * (o.upsample2 ? 2 : 1); }
            a.out = ptr(o.out); a.out_bstride = bstride(o.out); a.T_out = tlen(o.out);
            if (o.res != -1) { a.res = ptr(o.res); a.res_bstride = bstride(o.res); }
            a.alpha = o.alpha; a.beta = o.beta; a.acc_scale = o.acc_scale; a.out_act = o.out_act; a.out_slope = o.out_slope;
            a.out_transposed = o.out_transposed; a.B = B; a.tr_stride = o.tr_stride; a.tr_pad = o.tr_pad; a.tr_k = o.tr_k;
            // weights by format (vb_net_load checked the fields); launch_conv1d picks the kernel
            switch (o.wfmt) {
            case VB_WFMT_F32: a.w = o.w; break;
            case VB_WFMT_MF: a.w = o.w; a.w_mf = o.w_mf; break;      // w: the direct kernels where conv1d_f32w_kernel's run-time conditions fail
            case VB_WFMT_X3: {
                const int phases = o.tr_stride > 1 ? o.tr_stride : 1;
                const int ntaps = o.tr_stride > 1 ? (o.tr_k + o.tr_stride - 1) / o.tr_stride : o.ksize;
                a.w = o.w;                                            // (the one-output-channel kernel reads the fp32 copy)
                a.wp = (const bf16_t*)o.w_x3; a.Ci_pad = o.ci_pad; a.wp_plane = (int64_t)phases * ntaps * a.Co * o.ci_pad;
                break;
            }
            case VB_WFMT_BF16: {
                a.w = o.w;                                            // (Co = 1 only: the one-output-channel kernel's fp32 weights)
                a.wp = (const bf16_t*)o.w_x3; a.Ci_pad = o.ci_pad; a.wp_bf16 = true;         // (one plane: no plane stride)
                break;
            }
            case VB_WFMT_BUF_F32: a.w = ptr(o.w_buf); a.w_bstride = bstride(o.w_buf); break;
            case VB_WFMT_BUF_X3:
                // per-batch split planes [2][B][Co][Ci_pad] written by an earlier VB_OP_SPLIT_PLANES
                a.Ci_pad = (a.Ci + 31) / 32 * 32;
                a.wp = reinterpret_cast<const bf16_t*>(ptr(o.w_buf)); a.wp_bstride = (int64_t)a.Co * a.Ci_pad;
                a.wp_plane = (int64_t)B * a.wp_bstride;
                break;
            }
            VB_TRY(launch_conv1d(a, st));
        } else if (o.kind == VB_OP_GN_APPLY) {
            float* stp = ptr(o.stats);
            VB_TRY(launch_gn_apply(ptr(o.x), stp, stp + (size_t)B * o.gn_groups, o.gn_gamma, o.gn_beta, B, o.Ci, tlen(o.x), o.gn_groups,
                                   o.in_act == ACT_GN_SWISH ? 1 : 0, ptr(o.out), st, nl ? nl->table : nullptr, tmul(o.x)));
        } else if (o.kind == VB_OP_XT_PLANES) {
            const float* stp = o.stats >= 0 ? ptr(o.stats) : nullptr;
            VB_TRY(launch_xt_planes(ptr(o.x), stp, stp ? stp + (size_t)B * o.gn_groups : nullptr, o.gn_gamma, o.gn_beta, o.gn_groups, o.in_act, o.in_slope,
                                    o.upsample2, B, o.Ci, tlen(o.x), o.wfmt == VB_WFMT_BF16 ? 1 : 2, reinterpret_cast<bf16_t*>(ptr(o.out)), st,
                                    nl ? nl->table : nullptr, tmul(o.x) * (o.upsample2 ? 2 : 1)));
        } else if (o.kind == VB_OP_AA_ACT) {
            // (lengths: both filters replicate-pad at the row's own end, and the kernel writes the zeros behind it itself)
            VB_TRY(launch_aa_act(ptr(o.x), o.gn_gamma, o.gn_beta, o.w, B, o.Ci, tlen(o.x), ptr(o.out), st, nl ? nl->table : nullptr, tmul(o.x)));
        } else if (o.kind == VB_OP_RESPAIR) {
            if (o.wfmt == VB_WFMT_X3 || o.wfmt == VB_WFMT_BF16) {
                RespairArgs r;
                r.x = ptr(o.x); r.out = ptr(o.out); r.B = B; r.C = o.Ci; r.T = tlen(o.x); r.k = o.ksize; r.dil = o.dil;
                r.w1 = (const bf16_t*)o.w_x3; r.w2 = (const bf16_t*)o.w2; r.b1 = o.bias; r.b2 = o.bias2;
                r.slope = o.in_slope; r.alpha = o.alpha; r.beta = o.beta;
                if (nl) { r.row_len = nl->table; r.len_mul = tmul(o.x); }
                if (o.wfmt == VB_WFMT_BF16) VB_TRY(launch_respair_bf16(r, st));
                else VB_TRY(launch_respair(r, st));
            } else {
                RespairF32Args r;
                r.x = ptr(o.x); r.out = ptr(o.out); r.B = B; r.C = o.Ci; r.T = tlen(o.x); r.k = o.ksize; r.dil = o.dil;
                r.w1 = o.wfmt == VB_WFMT_MF ? o.w_mf : o.w; r.w2 = (const float*)o.w2; r.b1 = o.bias; r.b2 = o.bias2;
                r.slope = o.in_slope; r.alpha = o.alpha; r.beta = o.beta;
                if (nl) { r.row_len = nl->table; r.len_mul = tmul(o.x); }
                if (o.wfmt == VB_WFMT_MF) VB_TRY(launch_respair_f32w(r, st));
                else VB_TRY(launch_respair_f32(r, st));
            }
        } else if (o.kind == VB_OP_SPLIT_PLANES) {
            const int rows = o.Co > 0 ? o.Co : tlen(o.x), cols = o.Ci > 0 ? o.Ci : tlen(o.x);
            const int cpad = (cols + 31) / 32 * 32;
            VB_TRY(launch_split_rows(ptr(o.x), (int64_t)B * rows, cols, cpad, reinterpret_cast<bf16_t*>(ptr(o.out)), (int64_t)B * rows * cpad, st));
        } else {
            VB_FAIL(VB_E_INVALID, "net op %zu: bad kind %d", oi, o.kind);
        }
        // The tails of what the op wrote.  No pass: the planes of VB_OP_XT_PLANES (zero rows behind the row's end by its own bound) and of
        // VB_OP_SPLIT_PLANES (made from buffers whose tails are zero), the statistics, the transposed softmax (writes its zeros itself), the
        // anti-aliased activation (VB_OP_AA_ACT: with a length table its store bound is the row's own end and it writes exact zeros from
        // there to the pitch, whole workgroups of them before they load anything) and the square score buffer, of which the lengths
        // softmax reads the row's own block alone.  A transposed output [T][C] ends in the contiguous rows t >= len: one row of T * C
        // samples per clip.
        if (!nl || o.kind == VB_OP_XT_PLANES || o.kind == VB_OP_SPLIT_PLANES || o.kind == VB_OP_GN_STATS || o.kind == VB_OP_SOFTMAX_T
            || o.kind == VB_OP_AA_ACT)
            continue;
        if (o.out >= 0 && n.bufs[o.out].square == 1) continue;
        if (o.kind == VB_OP_CONV && o.out_transposed) VB_TRY(launch_tail_zero(ptr(o.out), nl->lp, nl->table, B, 1, T, tmul(o.out) * chans(o.out), st));
        else VB_TRY(launch_tail_zero(ptr(o.out), nl->lp, nl->table, B, chans(o.out), T, tmul(o.out), st));
    }
    return VB_OK;
}
// What a program must be to take row lengths, per net.  The vocoder (include/versband_hip.h, vb_hifigan_forward_lens) works by zero tails
// alone: every op computes a sample from a zero-padded window of its own row, through an input activation with f(0) = 0, into a plain
// [B][C][T] buffer.  The VAE decoder (vb_vae_decode_lens) adds what net_run gives a length table to - GroupNorm statistics and inputs, the
// attention's dynamic channel counts, w_buf weights, transposed outputs - and refuses whatever its program does not contain.  BigVGAN
// (vb_bigvgan_forward_lens) is the vocoder's contract plus VB_OP_AA_ACT, whose kernel takes the row's own end from the length table; the
// HiFi-GAN entry points keep refusing that op, so what they accept is what they accepted before the kernel learned it.  The VAE encoder
// (vb_vae_encode_lens) is the decoder's contract, turned round at the one op that changes the row's rate: it refuses upsample2 and admits
// in_stride > 1 on a convolution with no input activation and no statistics - Downsample1D as two polyphase sums, which net_run gives no
// length table (conv1d's refusal of row_len with in_stride stays): the right pad of the reference is the zeroed tail of the buffer they
// read, and the tail pass after each of the two keeps the output's own tail zero (the second adds w1 * 0, no bias, to a zeroed tail).
enum { LENS_VAE_DECODER = 0, LENS_VOCODER = 1, LENS_BIGVGAN = 2, LENS_VAE_ENCODER = 3 };
static int net_lens_check(const NetProgram& n, int contract) {
    const char* const fn = contract == LENS_BIGVGAN ? "bigvgan_forward_lens" : "hifigan_forward_lens";
    static const char* const kinds[] = {"VB_OP_CONV", "VB_OP_GN_STATS", "VB_OP_SOFTMAX_T", "VB_OP_SPLIT_PLANES", "VB_OP_RESPAIR", "VB_OP_GN_APPLY",
                                        "VB_OP_AA_ACT", "VB_OP_XT_PLANES"};
    for (size_t oi = 0; oi < n.ops.size(); ++oi) {
        const vb_net_op& o = n.ops[oi];
        const char* kn = o.kind >= 0 && o.kind <= VB_OP_XT_PLANES ? kinds[o.kind] : "unknown kind";
        if (contract == LENS_VAE_DECODER) {
            if (o.kind == VB_OP_AA_ACT)
                VB_FAIL(VB_E_INVALID, "vae_decode_lens: op %zu (%s): its anti-aliasing filters replicate-pad at the row end, which row lengths do not describe", oi, kn);
            if (o.kind == VB_OP_RESPAIR || o.kind < 0 || o.kind > VB_OP_XT_PLANES)
                VB_FAIL(VB_E_INVALID, "vae_decode_lens: op %zu (%s): not an op of the VAE decoder's program", oi, kn);
            if (o.kind == VB_OP_CONV && o.in_stride > 1)
                VB_FAIL(VB_E_INVALID, "vae_decode_lens: op %zu (%s): in_stride = %d reads across the row's own end (the encoder's down-convolutions)", oi, kn, o.in_stride);
            if (o.kind == VB_OP_CONV && o.tr_stride > 1)
                VB_FAIL(VB_E_INVALID, "vae_decode_lens: op %zu (%s): a transposed convolution (tr_stride = %d) is not an op of the VAE decoder's program", oi, kn, o.tr_stride);
            continue;
        }
        if (contract == LENS_VAE_ENCODER) {
            if (o.kind == VB_OP_AA_ACT || o.kind == VB_OP_RESPAIR || o.kind < 0 || o.kind > VB_OP_XT_PLANES)
                VB_FAIL(VB_E_INVALID, "vae_encode_lens: op %zu (%s): not an op of the VAE encoder's program", oi, kn);
            if ((o.kind == VB_OP_CONV || o.kind == VB_OP_XT_PLANES) && o.upsample2)
                VB_FAIL(VB_E_INVALID, "vae_encode_lens: op %zu (%s): upsample2 is not an op of the VAE encoder's program", oi, kn);
            if (o.kind == VB_OP_CONV && o.tr_stride > 1)
                VB_FAIL(VB_E_INVALID, "vae_encode_lens: op %zu (%s): a transposed convolution (tr_stride = %d) is not an op of the VAE encoder's program", oi, kn, o.tr_stride);
            if (o.in_stride > 1 && o.kind != VB_OP_CONV)
                VB_FAIL(VB_E_INVALID, "vae_encode_lens: op %zu (%s): in_stride = %d on an op that is not a convolution", oi, kn, o.in_stride);
            if (o.kind == VB_OP_CONV && o.in_stride > 1 && (o.in_act != ACT_NONE || o.stats != -1))
                VB_FAIL(VB_E_INVALID, "vae_encode_lens: op %zu (%s): in_stride = %d with input activation %d / statistics %d: an activated down-convolution "
                        "pads the ACTIVATED row, which a zero tail does not stand in for (none and -1 only)", oi, kn, o.in_stride, o.in_act, o.stats);
            continue;
        }
        if (o.kind == VB_OP_AA_ACT && contract == LENS_BIGVGAN) {
            // (out = f(x) of the row's own samples, no weights of a whole row, no statistics: all it needs is a plain [B][C][T] pair of buffers)
            if (o.Ci <= 0 || (o.x >= 0 && n.bufs[o.x].square != 0) || (o.out >= 0 && n.bufs[o.out].square != 0))
                VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): Ci = %d, or a buffer that is not [B][C][T]", fn, oi, kn, o.Ci);
            continue;
        }
        if (o.kind == VB_OP_AA_ACT)
            VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): its anti-aliasing filters replicate-pad at the row end, which a zero tail cannot stand in for", fn, oi, kn);
        if (o.kind != VB_OP_CONV && o.kind != VB_OP_RESPAIR && o.kind != VB_OP_XT_PLANES)
            VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): only VB_OP_CONV, VB_OP_RESPAIR and VB_OP_XT_PLANES%s take row lengths", fn, oi, kn,
                    contract == LENS_BIGVGAN ? " (and VB_OP_AA_ACT)" : "");
        if (o.in_act != ACT_NONE && o.in_act != ACT_LRELU)
            VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): input activation %d does not map 0 to 0 (none / LeakyReLU only)", fn, oi, kn, o.in_act);
        if (o.stats != -1) VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): GroupNorm statistics run over the whole row", fn, oi, kn);
        if (o.Ci <= 0 || (o.kind != VB_OP_XT_PLANES && o.Co <= 0))
            VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): a dynamic channel count (Ci = %d, Co = %d) contracts over the row length", fn, oi, kn, o.Ci, o.Co);
        if (o.w_buf != -1) VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): w_buf weights are made from whole rows", fn, oi, kn);
        if (o.out_transposed) VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): a transposed output is not a [B][C][T] buffer", fn, oi, kn);
        if (o.kind != VB_OP_XT_PLANES && o.out >= 0 && n.bufs[o.out].square != 0)
            VB_FAIL(VB_E_INVALID, "%s: op %zu (%s): writes a buffer of square = %d, not [B][C][T]", fn, oi, kn, n.bufs[o.out].square);
    }
    return VB_OK;
}

// The lengths entry points as data, one row per contract of net_lens_check: the net it runs, its own name (also its profiler range; messages
// drop the "vb_") and what messages call the net; chunked: the entry point that runs the same contract chunk by chunk, where there is one.
struct LensEntry { int which, contract; const char* name; const char* net; const char* chunked; };
static const LensEntry LENS_ENTRIES[] = {
    {VB_NET_VAE, LENS_VAE_DECODER, "vb_vae_decode_lens", "VAE decoder", nullptr},
    {VB_NET_VOCODER, LENS_VOCODER, "vb_hifigan_forward_lens", "vocoder", "vb_hifigan_forward_chunked_lens"},
    {VB_NET_VOCODER, LENS_BIGVGAN, "vb_bigvgan_forward_lens", "vocoder", "vb_bigvgan_forward_chunked_lens"},
    {VB_NET_VAE_ENCODER, LENS_VAE_ENCODER, "vb_vae_encode_lens", "VAE encoder", nullptr}};
static const char* fn_of(const char* name) { return name + 3; }

// The one lengths path of the nets, behind every row of LENS_ENTRIES.  Workspace: the net's own, the masked input, the table of row lengths.
static size_t net_lens_ws_bytes(vb_ctx* ctx, int which, int B, int T) {
    if (!ctx || !ctx->nets[which].loaded || B < 1 || T < 1) return 0;
    const NetProgram& n = ctx->nets[which];
    return net_ws_bytes(n, B, T, nullptr) + align_up((size_t)B * n.in_ch * T * n.in_tmul * sizeof(float)) + align_up(64 * sizeof(int));
}
static int net_run_lens(vb_ctx* ctx, const LensEntry& e, const float* in, int B, int T, const vb_lens* lens, float* out, void* ws, hipStream_t st) {
    const char* const fn = fn_of(e.name);
    if (!ctx) VB_FAIL(VB_E_INVALID, "%s: null ctx", fn);
    RoctxRange rr(e.name);
    NetLens nl;
    if (lens && lens->len) VB_TRY(lens_plan(lens->len, B, T, &nl.lp));
    if (!nl.lp.B) return net_run(ctx, e.which, in, B, T, out, ws, st);                 // no lengths, or every row full: the plain entry point
    NetProgram& n = ctx->nets[e.which];
    if (!n.loaded) VB_FAIL(VB_E_STATE, "%s: no %s loaded", fn, e.net);
    VB_TRY(net_lens_check(n, e.contract));
    // (the encoder alone takes its input at in_tmul samples per unit of len: T and len count latent tokens, row b owns len[b] * in_tmul frames)
    if (n.in_tmul != 1 && e.contract != LENS_VAE_ENCODER) VB_FAIL(VB_E_INVALID, "%s: the %s's input runs at %d samples per frame (1)", fn, e.net, n.in_tmul);
    VB_HIP(hipSetDevice(ctx->device));
    char* p = static_cast<char*>(ws) + net_ws_bytes(n, B, T, nullptr);
    float* masked = reinterpret_cast<float*>(p);
    int* table = reinterpret_cast<int*>(p + align_up((size_t)B * n.in_ch * T * n.in_tmul * sizeof(float)));
    VB_TRY(launch_lens_table(nl.lp, table, st));
    nl.table = table;
    VB_TRY(launch_mask_latent(in, B, n.in_ch, T * n.in_tmul, table, masked, st, n.in_tmul));      // (a select: the caller's padding, NaN included, is not read)
    return net_run(ctx, e.which, masked, B, T, out, ws, st, &nl);
}

// The plan of the chunked vocoder with row lengths (include/versband_hip.h, vb_hifigan_forward_chunked_lens): the chunk grid of
// vb_hifigan_forward_chunked - T <= chunk + 2 * halo is one step over the whole rows, as there - and per step the rows that have not ended
// before it with their frames inside it.  The one function behind the entry point and vb_hifigan_chunked_lens_plan.  len: HOST array;
// lens: the checked lengths (B = 0 in it when every row is full), for the caller that wants them.
struct ChunkStep { int s, e, lo, tc; ChunkRows rows; };
static int chunk_lens_plan(int B, int T, int chunk, int halo, const int32_t* len, std::vector<ChunkStep>* out, LensPlan* lens = nullptr) {
    if (chunk < 1 || halo < 0) VB_FAIL(VB_E_INVALID, "hifigan_forward_chunked_lens: chunk=%d halo=%d", chunk, halo);
    if (T < 1) VB_FAIL(VB_E_INVALID, "hifigan_forward_chunked_lens: T=%d", T);
    LensPlan lp;
    VB_TRY(lens_plan(len, B, T, &lp));                 // (B <= 64, 1 <= len[b] <= T: the row is named)
    if (lens) *lens = lp;
    out->clear();
    const bool whole = T <= (int64_t)chunk + 2 * (int64_t)halo;
    for (int64_t s64 = 0; s64 < T; s64 += whole ? T : chunk) {
        const int s = (int)s64;
        ChunkStep c;
        c.s = s;
        c.e = whole ? T : (int)std::min<int64_t>(s64 + chunk, T);
        c.lo = whole ? 0 : std::max(0, s - halo);
        c.tc = 0;
        const int64_t hi = whole ? T : s64 + chunk + halo;
        for (int b = 0; b < B; ++b) {
            if (len[b] <= s) continue;
            const int j = c.rows.n_active++;
            c.rows.row[j] = b;
            c.rows.n[j] = (int)std::min<int64_t>(len[b], hi) - c.lo;
            c.tc = std::max(c.tc, c.rows.n[j]);
        }
        out->push_back(c);
    }
    return VB_OK;
}

// the weight fields each allowed (kind, wfmt) pair of include/versband_hip.h reads; -1 = the pair is not allowed
enum { NW_W = 1, NW_X3 = 2, NW_MF = 4, NW_W2 = 8, NW_BUF = 16 };
static int net_op_fields(int kind, int wfmt, int Co) {
    switch (kind) {
    case VB_OP_CONV:
        switch (wfmt) {
        case VB_WFMT_F32: return NW_W;
        case VB_WFMT_X3: return NW_X3 | NW_W;
        case VB_WFMT_MF: return NW_MF | NW_W;
        case VB_WFMT_BF16: return NW_X3 | (Co == 1 ? NW_W : 0);
        case VB_WFMT_BUF_F32: case VB_WFMT_BUF_X3: return NW_BUF;
        }
        return -1;
    case VB_OP_RESPAIR:
        switch (wfmt) {
        case VB_WFMT_F32: return NW_W | NW_W2;
        case VB_WFMT_X3: return NW_X3 | NW_W2;
        case VB_WFMT_MF: return NW_MF | NW_W2;
        case VB_WFMT_BF16: return NW_X3 | NW_W2;
        }
        return -1;
    case VB_OP_AA_ACT: return wfmt == VB_WFMT_NONE ? NW_W : -1;
    case VB_OP_XT_PLANES: return wfmt == VB_WFMT_NONE || wfmt == VB_WFMT_BF16 ? 0 : -1;      // (BF16: the one-plane form; no weights either way)
    case VB_OP_GN_STATS: case VB_OP_SOFTMAX_T: case VB_OP_SPLIT_PLANES: case VB_OP_GN_APPLY:
        return wfmt == VB_WFMT_NONE ? 0 : -1;
    }
    return -1;
}

// The chunked vocoder with row lengths, behind the `chunked` entry points of LENS_ENTRIES: one plan, one gather / scatter, one loop.
static int chunked_lens_run(vb_ctx* ctx, const LensEntry& e, const float* mel, int B, int T, int chunk, int halo, const vb_lens* lens, float* wav,
                            void* ws, float* scratch_in, float* scratch_out, void* stream) {
    const char* const fn = fn_of(e.chunked);
    if (!ctx) VB_FAIL(VB_E_INVALID, "%s: null ctx", fn);
    if (chunk < 1 || halo < 0) VB_FAIL(VB_E_INVALID, "%s: chunk=%d halo=%d", fn, chunk, halo);
    NetProgram& net = ctx->nets[e.which];
    if (!net.loaded) VB_FAIL(VB_E_INVALID, "%s: no vocoder loaded", fn);
    if (!lens || !lens->len) return vb_hifigan_forward_chunked(ctx, mel, B, T, chunk, halo, wav, ws, scratch_in, scratch_out, stream);
    std::vector<ChunkStep> plan;
    LensPlan lp;
    VB_TRY(chunk_lens_plan(B, T, chunk, halo, lens->len, &plan, &lp));
    if (!lp.B) return vb_hifigan_forward_chunked(ctx, mel, B, T, chunk, halo, wav, ws, scratch_in, scratch_out, stream);      // every row full
    hipStream_t st = (hipStream_t)stream;
    if (T <= (int64_t)chunk + 2 * (int64_t)halo) return net_run_lens(ctx, e, mel, B, T, lens, wav, ws, st);                  // whole rows
    VB_TRY(net_lens_check(net, e.contract));
    if (net.in_tmul != 1) VB_FAIL(VB_E_INVALID, "%s: the vocoder's input runs at %d samples per frame (1)", fn, net.in_tmul);
    RoctxRange rr(e.chunked);
    VB_HIP(hipSetDevice(ctx->device));
    const int hop = net.out_tmul;
    int* table = reinterpret_cast<int*>(static_cast<char*>(ws) + net_ws_bytes(net, B, chunk + 2 * halo, nullptr));
    for (const ChunkStep& c : plan) {
        // the rows that reach into the chunk, compact and masked at their own ends; the generator on them with their in-chunk lengths (the
        // plain run when all are full); samples [s, e) * hop of every row of wav: its own, then zeros
        ChunkScatter cs;
        cs.n_active = c.rows.n_active;
        for (int b = 0; b < 64; ++b) cs.slot[b] = -1;
        NetLens nl;
        bool short_row = false;
        for (int j = 0; j < c.rows.n_active; ++j) {
            const int b = c.rows.row[j];
            cs.slot[b] = j;
            cs.keep[b] = std::min(c.e, (int)lens->len[b]) - c.s;
            nl.lp.len[j] = c.rows.n[j];
            short_row = short_row || c.rows.n[j] != c.tc;
        }
        if (c.rows.n_active > 0) {
            VB_TRY(launch_chunk_gather(mel, c.rows, net.in_ch, T, c.lo, c.tc, scratch_in, st));
            if (short_row) {
                nl.lp.B = c.rows.n_active;
                VB_TRY(launch_lens_table(nl.lp, table, st));
                nl.table = table;
            }
            VB_TRY(net_run(ctx, e.which, scratch_in, c.rows.n_active, c.tc, scratch_out, ws, st, short_row ? &nl : nullptr));
        }
        VB_TRY(launch_chunk_scatter(scratch_out, cs, B, net.out_ch, T, hop, c.s, c.e, c.lo, c.tc, wav, st));
    }
    return VB_OK;
}

extern "C" {

int vb_net_load(vb_ctx* ctx, int which, const vb_net_op* ops, int n_ops, const vb_buf_desc* bufs, int n_bufs, int in_channels,
                int out_channels, int in_tmul, int out_tmul) {
    if (!ctx || which < 0 || which > 2 || !ops || n_ops < 1 || in_tmul < 1 || out_tmul < 1) VB_FAIL(VB_E_INVALID, "net_load: bad argument");
    auto tmul = [&](int id) { return id == VB_BUF_INPUT ? in_tmul : (id == VB_BUF_OUTPUT ? out_tmul : bufs[id].tmul); };
    for (int i = 0; i < n_ops; ++i) {
        const vb_net_op& o = ops[i];
        const int ids[5] = {o.x, o.out, o.res, o.stats, o.w_buf};
        for (int id : ids)
            if (id >= n_bufs || (id < -3)) VB_FAIL(VB_E_INVALID, "net_load: op %d references buffer %d of %d", i, id, n_bufs);
        const int f = net_op_fields(o.kind, o.wfmt, o.Co);
        if (f < 0) VB_FAIL(VB_E_INVALID, "net_load: op %d: kind %d has no weight format %d", i, o.kind, o.wfmt);
        const struct { int bit; bool set; const char* name; } slots[] = {
            {NW_W, o.w != nullptr, "w"}, {NW_X3, o.w_x3 != nullptr, "w_x3"}, {NW_MF, o.w_mf != nullptr, "w_mf"}, {NW_W2, o.w2 != nullptr, "w2"},
            {NW_BUF, o.w_buf != -1, "w_buf"}};
        for (const auto& sl : slots)
            if (sl.set != ((f & sl.bit) != 0))
                VB_FAIL(VB_E_INVALID, "net_load: op %d (kind %d, weight format %d): %s is %s", i, o.kind, o.wfmt, sl.name,
                        sl.set ? "set but not read" : "missing");
        if ((f & NW_X3) && o.ci_pad != (o.Ci + 31) / 32 * 32)       // (the ops that read w_x3; a BF16 XT_PLANES has no weights)
            VB_FAIL(VB_E_INVALID, "net_load: op %d: split weights padded to %d input channels, not %d rounded up to 32", i, o.ci_pad, o.Ci);
        if (o.wfmt == VB_WFMT_MF && (!aligned16(o.w_mf) || !aligned16(o.w2)))
            VB_FAIL(VB_E_INVALID, "net_load: op %d: minimal-filtering weights are not 16-byte aligned", i);
        // DMA-fed input planes: the buffer holds as many planes as the reader's weight format multiplies (square 3 = two, 4 = one)
        if (o.kind == VB_OP_XT_PLANES) {
            const int want = o.wfmt == VB_WFMT_BF16 ? 4 : 3;
            if (o.out < 0 || bufs[o.out].square != want)
                VB_FAIL(VB_E_INVALID, "net_load: op %d: %s planes are written to a buffer of square = %d", i, want == 4 ? "one-plane (BF16)" : "split", want);
        }
        if (o.kind == VB_OP_CONV && o.x_planes) {
            const int sq = o.x >= 0 ? bufs[o.x].square : 0;
            if (o.wfmt == VB_WFMT_X3 ? sq != 3 : (o.wfmt == VB_WFMT_BF16 ? sq != 4 : true))
                VB_FAIL(VB_E_INVALID, "net_load: op %d: x_planes with weight format %d reads a buffer of square = %d (X3: 3, split planes; BF16: 4, one plane)",
                        i, o.wfmt, sq);
            if (o.wfmt == VB_WFMT_BF16 && o.Co == 1)
                VB_FAIL(VB_E_INVALID, "net_load: op %d: one output channel runs the fp32 one-output-channel kernel, which reads no planes", i);
        }
        if (o.kind == VB_OP_RESPAIR) {
            if (!o.bias || !o.bias2) VB_FAIL(VB_E_INVALID, "net_load: op %d: respair without both biases", i);
            if (o.Ci != o.Co) VB_FAIL(VB_E_INVALID, "net_load: op %d: respair with Ci %d != Co %d", i, o.Ci, o.Co);
            if (o.wfmt == VB_WFMT_BF16 && o.Ci != 32 && o.Ci != 64) VB_FAIL(VB_E_INVALID, "net_load: op %d: bf16 respair with %d channels (32 or 64)", i, o.Ci);
            if (o.x == -1 || o.out == -1 || tmul(o.x) != tmul(o.out))
                VB_FAIL(VB_E_INVALID, "net_load: op %d: respair input and output differ in length", i);
        }
    }
    NetProgram& n = ctx->nets[which];
    n.ops.assign(ops, ops + n_ops);
    n.bufs.assign(bufs, bufs + n_bufs);
    n.in_ch = in_channels; n.out_ch = out_channels; n.in_tmul = in_tmul; n.out_tmul = out_tmul; n.loaded = true;
    return VB_OK;
}
size_t vb_net_workspace_bytes(vb_ctx* ctx, int which, int B, int T) {
    if (!ctx || which < 0 || which > 2 || !ctx->nets[which].loaded) return 0;
    return net_ws_bytes(ctx->nets[which], B, T, nullptr);
}
int vb_vae_decode(vb_ctx* ctx, const float* z, int B, int T, float* mel, void* ws, void* stream) {
    if (!ctx) VB_FAIL(VB_E_INVALID, "vae_decode: null ctx");
    RoctxRange rr("vb_vae_decode");
    return net_run(ctx, VB_NET_VAE, z, B, T, mel, ws, (hipStream_t)stream);
}
int vb_vae_encode(vb_ctx* ctx, const float* mel, int B, int T, float* moments, void* ws, void* stream) {
    if (!ctx) VB_FAIL(VB_E_INVALID, "vae_encode: null ctx");
    RoctxRange rr("vb_vae_encode");
    return net_run(ctx, VB_NET_VAE_ENCODER, mel, B, T, moments, ws, (hipStream_t)stream);
}
int vb_hifigan_forward(vb_ctx* ctx, const float* mel, int B, int T, float* wav, void* ws, void* stream) {
    if (!ctx) VB_FAIL(VB_E_INVALID, "hifigan_forward: null ctx");
    RoctxRange rr("vb_hifigan_forward");
    return net_run(ctx, VB_NET_VOCODER, mel, B, T, wav, ws, (hipStream_t)stream);
}
size_t vb_hifigan_lens_workspace_bytes(vb_ctx* ctx, int B, int T) { return net_lens_ws_bytes(ctx, LENS_ENTRIES[LENS_VOCODER].which, B, T); }
int vb_hifigan_forward_lens(vb_ctx* ctx, const float* mel, int B, int T, const vb_lens* lens, float* wav, void* ws, void* stream) {
    return net_run_lens(ctx, LENS_ENTRIES[LENS_VOCODER], mel, B, T, lens, wav, ws, (hipStream_t)stream);
}
size_t vb_vae_decode_lens_workspace_bytes(vb_ctx* ctx, int B, int T) { return net_lens_ws_bytes(ctx, LENS_ENTRIES[LENS_VAE_DECODER].which, B, T); }
int vb_vae_decode_lens(vb_ctx* ctx, const float* z, int B, int T, const vb_lens* lens, float* mel, void* ws, void* stream) {
    return net_run_lens(ctx, LENS_ENTRIES[LENS_VAE_DECODER], z, B, T, lens, mel, ws, (hipStream_t)stream);
}
size_t vb_vae_encode_lens_workspace_bytes(vb_ctx* ctx, int B, int T) { return net_lens_ws_bytes(ctx, LENS_ENTRIES[LENS_VAE_ENCODER].which, B, T); }
int vb_vae_encode_lens(vb_ctx* ctx, const float* mel, int B, int T, const vb_lens* lens, float* moments, void* ws, void* stream) {
    return net_run_lens(ctx, LENS_ENTRIES[LENS_VAE_ENCODER], mel, B, T, lens, moments, ws, (hipStream_t)stream);
}
int vb_posterior_lens(const float* moments, const float* noise, int B, int E, int T, const int32_t* len, float scale, float* z, void* stream) {
    if (!moments || !z || B < 1 || E < 1 || T < 1) VB_FAIL(VB_E_INVALID, "posterior_lens: null pointer or B/E/T < 1");
    LensPlan lp;
    if (len) VB_TRY(lens_plan(len, B, T, &lp));      // (B <= 64, 1 <= len[b] <= T: the row is named; B = 0 in lp: every row full)
    return launch_posterior_lens(moments, noise, B, E, T, lp, scale, z, (hipStream_t)stream);
}
int vb_crossfade_windows(const float* parts, const int32_t* starts, int nw, int B, int C, int n, int T, float* out, void* stream) {
    if (!parts || !starts || !out || nw < 1 || B < 1 || C < 1 || n < 1 || T < 1) VB_FAIL(VB_E_INVALID, "crossfade_windows: null pointer or nw/B/C/n/T < 1");
    return launch_crossfade_windows(parts, starts, nw, B, C, n, T, out, (hipStream_t)stream);
}
int vb_hifigan_forward_chunked(vb_ctx* ctx, const float* mel, int B, int T, int chunk, int halo, float* wav, void* ws, float* scratch_in,
                               float* scratch_out, void* stream) {
    if (!ctx) VB_FAIL(VB_E_INVALID, "hifigan_forward_chunked: null ctx");
    if (chunk < 1 || halo < 0) VB_FAIL(VB_E_INVALID, "hifigan_forward_chunked: chunk=%d halo=%d", chunk, halo);
    NetProgram& n = ctx->nets[VB_NET_VOCODER];
    if (!n.loaded) VB_FAIL(VB_E_STATE, "hifigan_forward_chunked: no vocoder loaded");
    hipStream_t st = (hipStream_t)stream;
    RoctxRange rr("vb_hifigan_forward_chunked");
    if (T <= chunk + 2 * halo) return net_run(ctx, VB_NET_VOCODER, mel, B, T, wav, ws, st);
    VB_HIP(hipSetDevice(ctx->device));
    const int hop = n.out_tmul, rows_in = B * n.in_ch, rows_out = B * n.out_ch;
    for (int s = 0; s < T; s += chunk) {
        // frames [lo, hi) = the chunk with its context; every row (clip, channel) of the slice is gathered into a contiguous tensor, the
        // generator runs on it, and the samples of [s, e) are scattered into the whole-clip waveform (strided 2-D copies, no kernel)
        const int e = s + chunk < T ? s + chunk : T;
        const int lo = s - halo > 0 ? s - halo : 0, hi = e + halo < T ? e + halo : T;
        const int tc = hi - lo;
        VB_HIP(hipMemcpy2DAsync(scratch_in, (size_t)tc * sizeof(float), mel + lo, (size_t)T * sizeof(float), (size_t)tc * sizeof(float), rows_in,
                                hipMemcpyDeviceToDevice, st));
        VB_TRY(net_run(ctx, VB_NET_VOCODER, scratch_in, B, tc, scratch_out, ws, st));
        VB_HIP(hipMemcpy2DAsync(wav + (size_t)s * hop, (size_t)T * hop * sizeof(float), scratch_out + (size_t)(s - lo) * hop,
                                (size_t)tc * hop * sizeof(float), (size_t)(e - s) * hop * sizeof(float), rows_out, hipMemcpyDeviceToDevice, st));
    }
    return VB_OK;
}
size_t vb_hifigan_chunked_lens_workspace_bytes(vb_ctx* ctx, int B, int T, int chunk, int halo) {
    if (!ctx || !ctx->nets[VB_NET_VOCODER].loaded || B < 1 || T < 1 || chunk < 1 || halo < 0) return 0;
    const int64_t tc = (int64_t)chunk + 2 * (int64_t)halo;
    if (T <= tc) return net_lens_ws_bytes(ctx, VB_NET_VOCODER, B, T);                   // (vb_hifigan_forward_lens, or the plain run, of the whole rows)
    return net_ws_bytes(ctx->nets[VB_NET_VOCODER], B, (int)tc, nullptr) + align_up(64 * sizeof(int));
}
int vb_hifigan_chunked_lens_plan(int B, int T, int chunk, int halo, const int32_t* len, int max_chunks, int32_t* s, int32_t* lo, int32_t* tc,
                                 int32_t* n_active, int32_t* rows, int32_t* n, int* n_chunks) {
    if (!s || !lo || !tc || !n_active || !rows || !n || !n_chunks || max_chunks < 0) VB_FAIL(VB_E_INVALID, "hifigan_chunked_lens_plan: null output or max_chunks < 0");
    std::vector<ChunkStep> plan;
    VB_TRY(chunk_lens_plan(B, T, chunk, halo, len, &plan));
    *n_chunks = (int)plan.size();
    if ((int64_t)plan.size() > max_chunks) VB_FAIL(VB_E_INVALID, "hifigan_chunked_lens_plan: %zu chunks, room for %d", plan.size(), max_chunks);
    for (size_t k = 0; k < plan.size(); ++k) {
        const ChunkStep& c = plan[k];
        s[k] = c.s; lo[k] = c.lo; tc[k] = c.tc; n_active[k] = c.rows.n_active;
        for (int j = 0; j < 64; ++j) {
            rows[k * 64 + j] = j < c.rows.n_active ? c.rows.row[j] : -1;
            n[k * 64 + j] = j < c.rows.n_active ? c.rows.n[j] : 0;
        }
    }
    return VB_OK;
}
size_t vb_bigvgan_lens_workspace_bytes(vb_ctx* ctx, int B, int T) { return net_lens_ws_bytes(ctx, LENS_ENTRIES[LENS_BIGVGAN].which, B, T); }
int vb_bigvgan_forward_lens(vb_ctx* ctx, const float* mel, int B, int T, const vb_lens* lens, float* wav, void* ws, void* stream) {
    return net_run_lens(ctx, LENS_ENTRIES[LENS_BIGVGAN], mel, B, T, lens, wav, ws, (hipStream_t)stream);
}
int vb_hifigan_forward_chunked_lens(vb_ctx* ctx, const float* mel, int B, int T, int chunk, int halo, const vb_lens* lens, float* wav, void* ws,
                                    float* scratch_in, float* scratch_out, void* stream) {
    return chunked_lens_run(ctx, LENS_ENTRIES[LENS_VOCODER], mel, B, T, chunk, halo, lens, wav, ws, scratch_in, scratch_out, stream);
}
size_t vb_bigvgan_chunked_lens_workspace_bytes(vb_ctx* ctx, int B, int T, int chunk, int halo) {
    return vb_hifigan_chunked_lens_workspace_bytes(ctx, B, T, chunk, halo);
}
int vb_bigvgan_forward_chunked_lens(vb_ctx* ctx, const float* mel, int B, int T, int chunk, int halo, const vb_lens* lens, float* wav, void* ws,
                                    float* scratch_in, float* scratch_out, void* stream) {
    return chunked_lens_run(ctx, LENS_ENTRIES[LENS_BIGVGAN], mel, B, T, chunk, halo, lens, wav, ws, scratch_in, scratch_out, stream);
}

}  // extern "C"
