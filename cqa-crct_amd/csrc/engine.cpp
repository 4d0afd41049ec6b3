// Step engine: schedules the hand-written gfx950 kernels for one CRCT training step
// (forward + joint loss + backward) on four HIP streams -- the caller's (text layers), one for the visual layers and one per data
// stream for its weight-gradient GEMMs, ordered by events -- without host synchronisation.
//
// Reference path it replaces (levymsn/CQA-CRCT):
//   encoder_decorator.forward            CRCT/backbone/encoder_decorator.py:73-158
//   BertForMultiModalPreTraining.forward CRCT/backbone/vilbert.py:1540-1661
//   BertModel.forward / BertEncoder      vilbert.py:1348-1441 / :822-946 (layer order :852-939)
//   BertLayer / BertImageLayer           vilbert.py:361-485 / :488-616
//   BertConnectionLayer                  vilbert.py:619-788
//   poolers, heads, regressor            vilbert.py:949-976, :1048-1062; regressor.py:5-42
//   + torch autograd of all of it (train.py:208).
//
// Data layout in HBM: parameters live in ONE flat fp32 buffer (and a bf16 shadow with identical
// element offsets) ordered by first use, so the gradient buffer completes back-to-front during
// backward and contiguous ranges can be all-reduced while earlier layers are still computing.
// query/key/value weights of a layer are adjacent -> one [3H, H] fused-QKV GEMM operand.
// Activations kept for backward are bf16 in a caller-provided workspace.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <functional>
#include <vector>

#include "crct_internal.h"

typedef unsigned short bf16_t;
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_LEAKY = 3, ACT_TANH = 4 };

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
void crct_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* crct_last_error(void) { return g_err; }
extern "C" int crct_abi_version(void) { return 7; }

// What every GEMM launch must satisfy, stated once: `who` prefixes the message ("gemm" / "gemm_grouped"), idx >= 0 names the
// problem of a grouped launch.  ln: the problem's LayerNorm addend, or NULL for none.
static int gemm_check(const CrctGemmArgs& a, const CrctGemmLnAddend* ln, const char* who, int idx) {
  char of[32] = "";
  if (idx >= 0) snprintf(of, sizeof(of), " (problem %d)", idx);
  CRCT_REQUIRE(a.A && a.B && a.C, "%s: null operand%s", who, of);
  CRCT_REQUIRE(a.N % 4 == 0, "%s: N=%d must be a multiple of 4%s", who, a.N, of);
  CRCT_REQUIRE((a.ta && a.tb) || a.K % 8 == 0, "%s: K=%d must be a multiple of 8 for a K-contiguous operand%s", who, a.K, of);
  CRCT_REQUIRE(a.lda % 8 == 0 && a.ldb % 8 == 0, "%s: lda=%ld ldb=%ld must be multiples of 8%s", who, (long)a.lda, (long)a.ldb, of);
  CRCT_REQUIRE(a.ldc % 4 == 0, "%s: ldc=%ld must be a multiple of 4%s", who, (long)a.ldc, of);
  CRCT_REQUIRE(!(a.ta && !a.tb), "%s: (ta=1, tb=0) is not built (not used by the step)%s", who, of);
  CRCT_REQUIRE(!a.ta || a.M % 8 == 0, "%s: transposed A needs M %% 8 == 0 (M=%d)%s", who, a.M, of);
  CRCT_REQUIRE(!a.tb || a.N % 8 == 0, "%s: transposed B needs N %% 8 == 0 (N=%d)%s", who, a.N, of);
  CRCT_REQUIRE(a.tile < 0 || crct_gemm_config_built(a.tile), "%s: configuration %d is not built%s", who, a.tile, of);
  // the staged epilogue stores a c_cached output without reading it, the register-staged one adds the old value: refused on both paths
  CRCT_REQUIRE(!(a.c_cached && a.accumulate), "%s: c_cached with accumulate is not supported (c_cached is a plain fp32 store)%s", who, of);
  // a LayerNorm addend stands on the fp32 addend it normalises and needs all four of its vectors.  (An fp8 weight gradient takes no
  // addend of any kind: gemm.hip, f8t_ok refuses a.addend, and with it this one.)
  CRCT_REQUIRE(!ln || (a.addend && a.addend_f32 && ln->mean && ln->rstd && ln->gamma && ln->beta),
               "%s: a LayerNorm addend needs the fp32 addend it normalises (addend, addend_f32) and mean, rstd, gamma, beta%s", who, of);
  return 0;
}

extern "C" int crct_gemm_bf16_ln_addend(const CrctGemmArgs* a, const CrctGemmLnAddend* ln, crct_stream_t stream) {
  CRCT_REQUIRE(a != nullptr, "gemm: null args");
  if (int r = gemm_check(*a, ln, "gemm", -1)) return r;
  CRCT_CHECK_HIP(crct_gemm_launch(*a, ln, (hipStream_t)stream));
  return 0;
}
extern "C" int crct_gemm_bf16(const CrctGemmArgs* a, crct_stream_t stream) { return crct_gemm_bf16_ln_addend(a, nullptr, stream); }

static int gemm_grouped_checked(const CrctGemmGroup& grp, crct_stream_t stream) {
  CRCT_REQUIRE(grp.gs != nullptr && grp.n >= 1, "gemm_grouped: bad arguments");
  for (int i = 0; i < grp.n; ++i)
    if (int r = gemm_check(grp.gs[i], grp.ln && grp.ln[i].mean ? &grp.ln[i] : nullptr, "gemm_grouped", i)) return r;      // mean == NULL: none for this problem
  CRCT_CHECK_HIP(crct_gemm_launch_grouped(grp, (hipStream_t)stream));
  return 0;
}
extern "C" int crct_gemm_bf16_grouped_ln_addend(const CrctGemmArgs* a, const CrctGemmLnAddend* ln, int n, crct_stream_t stream) {
  return gemm_grouped_checked(CrctGemmGroup{a, ln, n, nullptr, -1}, stream);      // -1: the library's default grid policy
}
extern "C" int crct_gemm_bf16_grouped(const CrctGemmArgs* a, int n, crct_stream_t stream) { return crct_gemm_bf16_grouped_ln_addend(a, nullptr, n, stream); }

namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline uint32_t thr_of(float p) {
  double t = (double)p * 4294967296.0;
  if (t <= 0.0) return 0u;
  if (t >= 4294967295.0) return 4294967295u;
  return (uint32_t)t;
}

struct Arena {
  size_t top = 0;
  size_t take(size_t bytes) { size_t o = top; top = align_up(top + bytes, 256); return o; }
};

struct Drop { uint32_t thr = 0; float scale = 1.f; uint32_t site = 0; };
inline Drop drop_of(const CrctStepCfg* c, float p, uint32_t site) {      // dropout p at `site` under step configuration c: off outside training
  Drop d; d.site = site;
  if (c->training && p > 0.f) { d.thr = thr_of(p); d.scale = 1.0f / (1.0f - p); }
  return d;
}

// ---- parameter offsets (elements into the flat buffers)
struct LinearP { int64_t w = -1, b = -1; int in = 0, out = 0; int site = 0; int parts = 1; };      // parts: 3 for a fused QKV (three tensors back to back)
struct LnP { int64_t g = -1, b = -1; };
struct FfnP { LinearP up, down; LnP ln; };
struct ProjP { LinearP dense; LnP ln; };      // LN(dropout(dense(ctx)) + residual)
struct SelfLayerP { LinearP qkv; ProjP proj; FfnP ffn; int H, heads; float p_attn, p_hid; uint32_t site; };
struct ConnLayerP { LinearP qkv1, qkv2; ProjP proj_v, proj_t; FfnP ffn_v, ffn_t; uint32_t site; };

// ---- activation offsets (bytes into the workspace)
constexpr size_t NONE = (size_t)-1;
// An activation as the blocks hand it on: the bf16 tensor, its e4m3 copy with the activation scale site (site -1: no copy) and, for the
// fp32 residual stream, where the fp32 value of a LayerNorm's output comes from: s / mean / rstd / ln -- the rows the LayerNorm normalised,
// their statistics and its parameters, from which the block-closing GEMM rebuilds it (CrctGemmLnAddend) -- and x32, the fp32 copy the
// LayerNorm writes on the two-output route (crct_engine_set_ln_addend(e, 0)).  NONE: the embeddings' outputs, bf16 there.
struct Act { size_t x = 0, q = NONE; int site = -1; size_t x32 = NONE; size_t s = NONE, mean = NONE, rstd = NONE; LnP ln; };
// the e5m2 copy of a gradient and its gradient scale site (-1: no copy)
struct GradQ { size_t q = NONE; int site = -1; };
// s: the pre-LayerNorm sum, room for fp32 (the fp32 residual stream, CrctStepCfg.residual_fp32; bf16 in the first half otherwise);
// y32 / a32: the fp32 copy of the LayerNorm output that the NEXT block's epilogue adds as its residual on the two-output route (planned
// behind everything else: crct_engine_set_ln_addend)
// hq / yq: e4m3 copies (fp8 forward), site_*: their scale slots; g_*: gradient scale sites (fp8 backward)
struct FfnA {
  size_t u, h, s, y, y32, mean, rstd, hq, yq; int site_h, site_y; int g_dl, g_du;
  Act out(const LnP& ln) const { return {y, yq, site_y, y32, s, mean, rstd, ln}; }
};
struct ProjA {
  size_t s, a, a32, mean, rstd, aq; int site_a; int g_dl;
  Act out(const LnP& ln) const { return {a, aq, site_a, a32, s, mean, rstd, ln}; }
};
// ctxq / site_ctx: e4m3 copy of the attention context and its activation scale site; g_dqkv: gradient scale site of the fused dqkv buffer
// lse*: softmax row statistics [B][heads][Tq] fp32 the long-sequence attention forward leaves for its backward (CrctAttnQuant.row_lse)
struct SelfLayerA { size_t qkv, ctx, ctxq, lse; int site_ctx, g_dqkv; ProjA proj; FfnA ffn; };
struct ConnLayerA { size_t qkv1, qkv2, ctx1, ctx2, ctx1q, ctx2q, lse1, lse2; int site_ctx1, site_ctx2, g_dqkv1, g_dqkv2; ProjA proj_v, proj_t; FfnA ffn_v, ffn_t; };
struct StreamScratch { size_t dy[2], dres_a, dlin_a, dres_b, dlin_b, gc, du, dctx, dqkv, part_a, part_b, dlq_a, dlq_b, duq, dqkvq; };      // *q: e5m2 copies (fp8 backward)

struct Step { char kind; int idx; };
struct StepIn { Act t, v; };      // the two hidden states a schedule step starts from
struct Tap { std::string name; size_t off; char stream; int width = 0; };      // width: elements per row where it is not the stream's hidden size (the fused qkv buffers)
// What one backward segment does (crct_engine_backward_plan): whether it runs, whether the gradients of its text / visual
// input are produced (the embedding segment: whether that stream's half runs), how many weight-gradient GEMMs it leaves out
struct SegPlan { bool runs = true, dx_t = true, dx_v = true; int dropped = 0; };

// One attention of the schedule as every launch that touches it sees it (crct_engine::attn_site).  kind 0 / 1: self-attention of text /
// visual layer `index`; 2: connection layer, direction 0 = text queries over visual keys, 1 = visual queries over text keys.  q, k, v:
// workspace offsets of its columns in the fused q | k | v buffers (ld elements a row); image_keys: the IMAGE key mask, else the text one;
// p / site: attention dropout; lse: row statistics of the long kernels; ctx / ctxq / site_ctx: the context, its e4m3 copy and scale site
struct AttnSite {
  int kind = 0, index = 0, direction = 0;
  size_t q = 0, k = 0, v = 0; int64_t ld = 0;
  int heads = 0, d = 0, Tq = 0, Tk = 0;
  bool image_keys = false;
  float p = 0.f; uint32_t site = 0;
  size_t lse = NONE, ctx = 0, ctxq = NONE; int site_ctx = -1;
  int H() const { return heads * d; }
};

// The per-pass gradient requests, each standing until its setter (crct_engine_set_*_grads) replaces it; all NULL / empty: off.  ig: where
// backward leaves the gradients of the float inputs -- the one family replan reads; og / sg: upstream gradients of the final hidden states
// (segment 0 adds them onto the running hidden gradients) and of the logits and the regressed value (heads_bwd's loss kernel); amg: the maps
// whose upstream gradients are added behind their attention backward.  Workspace behind the plan's own `base` bytes: ws_ig, the fp32
// [maxB * maxV][Fv] upstream gradient of the feature softmax, counted while d_image_feat is requested; behind it the scratch of
// crct_attention_probs_bwd, ws_amg bytes per data stream (the two run side by side), counted while a map request stands
struct Requests {
  CrctInputGrads ig = {nullptr, nullptr, nullptr, nullptr, nullptr};
  CrctOutputGrads og = {nullptr, nullptr};
  CrctScoreGrads sg = {nullptr, nullptr};
  std::vector<CrctAttnMapGrad> amg;
  size_t ws_ig = 0, ws_amg = 0;
  bool ig_text() const { return ig.d_txt_loc || ig.d_text_emb; }
  bool ig_vis() const { return ig.d_image_feat || ig.d_image_loc || ig.d_areas; }
  size_t amg_scratch(size_t base, int which) const { return base + ws_ig + (size_t)which * ws_amg; }
  size_t ws_bytes(size_t base) const { return amg.empty() ? base + (ig.d_image_feat ? ws_ig : 0) : amg_scratch(base, 2); }
};

}  // namespace

struct crct_engine {
  CrctModelDims d;
  std::unordered_map<std::string, int64_t> off, size;
  int maxB, maxT, maxV;
  std::vector<Step> sched;
  std::vector<SelfLayerP> tl, vl;
  std::vector<ConnLayerP> cl;
  std::vector<SelfLayerA> tla, vla;
  std::vector<ConnLayerA> cla;
  struct { int64_t word, pos, type, wloc, bloc; LnP ln; } et;
  struct { LinearP img; int64_t color, wloc, bloc; LnP ln; LinearP areas; } ev;
  // model variant (crct_engine_create_variant): dataset / regressor kind and the value table; `feat` = the image features are embedded
  CrctVariant var = {CRCT_DATASET_PLOTQA, CRCT_REGRESSOR_PLOTQA, 0, {}};
  bool feat = true;
  const float* areas = nullptr;        // crct_engine_set_areas: fp32 [B][V] of the running batch, or NULL
  // the standing per-pass requests; the workspace is the plan's own bytes (ws_base) and what they add: the one place its size is set
  Requests req;
  size_t ws_base() const { return ln_addend ? ws_core : ws_two_output; }
  void ws_update() { ws_bytes = req.ws_bytes(ws_base()); }
  // whether a tensor WITH gradient sits in the text / image embedding (replan): an embedding half that runs for a requested input
  // gradient alone leaves the parameter-gradient kernels out
  bool emb_own_t = true, emb_own_v = true;
  int fwd_r32 = -1;      // residual_fp32 of the last forward (-1: none yet): whether crct_engine_sequence_outputs reads fp32 or bf16 rows
  int attn_site(const char* who, int kind, int index, int direction, int T, int V, AttnSite* out) const;
  struct { size_t sum, y, mean, rstd, yq; int site; } eta;
  struct { size_t soft, lin, sum, y, mean, rstd, yq; int site; } eva;
  LinearP t_pool, v_pool, cls, tp[4], vp[4], fu[4];
  struct { size_t pooled_t, pooled_v, t[3], v[3], cat, f[3], scratch, ce, d_pt, d_pv, g[10]; } ha;   // g: one buffer per head gradient (see heads_bwd)
  StreamScratch st, sv;          // backward scratch per data stream (dy ping-pong lives in these)
  StreamScratch st2, sv2;        // second set: layers alternate sets so weight-gradient GEMMs may lag one layer behind
  size_t partials[2], colsum_part[4];   // per internal stream: [text, visual] / [text, visual, text-wgrad, visual-wgrad]
  size_t embed_rows[2], embed_idx[2];   // embedding backward: fp32 row gradients + table indices for the gather-sum pass
  size_t km_t = 0, km_v = 0;
  // per-site launch policy of the forward / data-gradient GEMMs (crct_engine_set_site_policy): [site][kind][phase]
  struct SitePolicy { int cfg = -1, split_k = 0; };
  SitePolicy policy[CRCT_SITE_COUNT][3][2];      // kind 2 (weight gradient): cfg only -- the layer's grouped launch takes the first problem's
  size_t sk_ws[2] = {0, 0}, sk_cnt[2] = {0, 0};   // split-K slab space / ticket words per data stream [text, visual]
  size_t sk_ws_elems[2] = {0, 0};
  int sk_tickets = 0;
  // fp8 forward (BASELINE configs[4]): scale slot of every Linear weight that has an e4m3 shadow, number of activation scale sites
  std::unordered_map<int64_t, int> wq_slot;
  int32_t* word_index = nullptr;      // device memory owned by the engine: crct_embed_text_bwd_indexed's first / last row per token id, zero between calls
  std::vector<std::pair<int64_t, int64_t>> wq_list;      // slot -> (flat offset, numel)
  int n_sites = 0;
  int n_gsites = 0;                    // gradient scale sites of the fp8 backward (CrctStepCfg.fp8_grad_scale / _amax)
  size_t ws_bytes = 0;
  // internal concurrency: the visual stream's layers and all weight-gradient GEMMs run on side HIP
  // streams, ordered against the caller's stream by events (fork / join inside every call)
  bool use_vis_stream = true, use_wgrad_stream = true, streams_forced = false;
  int wgrad_target = 96, wgrad_target_rows = 3000;      // crct_engine_set_wgrad_workgroups (Run::flush_wgrads)
  int ln_addend = 1;                   // crct_engine_set_ln_addend: 1 = the block-closing GEMMs rebuild their fp32 addend (Run::residual), 0 = the LayerNorms write it
  size_t ws_core = 0, ws_two_output = 0;      // workspace bytes without / with the fp32 LayerNorm outputs of the two-output route
  int wgrad_flush = 1;                 // crct_engine_set_wgrad_flush: extra flush points of a layer's queued weight gradients (Run::ffn_bwd).
                                       // 1 (round 4): FFN group 0.075 -> 0.081 of peak in the step, step -0.02 (bf16) / -0.06 (fp8) / -0.08 ms (long context)
  bool one_wgrad_stream = false;       // both data streams' weight gradients on ONE side stream (frees a hardware queue for the exchange)
  int first_conn = -1;                  // schedule index of the first co-attention layer
  hipStream_t side[3] = {nullptr, nullptr, nullptr};   // visual, text-wgrad, visual-wgrad
  // hardware-queue placement (streams.hip): the four streams below sit on queues other than the caller's stream's -- visual and
  // text-wgrad on queues of their own, the auxiliary stream (optimizer overlap during forward, gradient exchange during
  // backward: crct_engine_aux_stream) on the third, which the visual-wgrad stream shares (it is idle whenever the optimizer
  // runs; with one_wgrad_stream it is not used and the exchange has that queue to itself)
  hipStream_t aux = nullptr;
  hipStream_t placed_for = nullptr;
  bool placed = false;
  int queue_classes = 0;
  std::vector<hipEvent_t> evpool;
  size_t evnext = 0;
  std::vector<std::pair<int64_t, int64_t>> seg_range;
  // 1: segment 0 is the masked-LM head's (cls.predictions.*, params['lm_loss_coeff'] > 0) and / or the masked-region head's
  // (cls.imagePredictions.*, params['img_loss_coeff'] > 0): its gradients are produced by the host side (csrc/lm_head.hip,
  // csrc/region_head.hip) before the pass starts, so it launches nothing here and only takes part in the events; the heads' segment and
  // everything behind it then sit one place further back.  0 (those tensors have size 0): segments and ranges as without it.
  int lm_seg = 0;
  // weight-gradient ownership (CrctStepCfg.wgrad_overwrite): the Linear weights whose gradient is produced by exactly ONE
  // weight-gradient GEMM per backward pass and by nothing else -- every Linear of the encoder layers, the image embedding,
  // the poolers and the regressor pipes.  Fixed by the schedule at crct_engine_create (offset -> numel); `wgrad_pass` counts
  // the productions of the running pass so that a violation is an error, never a silent overwrite.
  std::unordered_map<int64_t, int64_t> wgrad_owned;
  std::unordered_map<int64_t, int> wgrad_pass;
  void wgrad_pass_begin() { wgrad_pass.clear(); }
  // tensors without gradient (crct_engine_set_trainable): their flat offsets, and what backward leaves out because of them.  Empty
  // set = every tensor has a gradient: the plan is all-true and no launch or event differs.
  std::vector<int64_t> param_off;      // offsets in the order given to crct_engine_create*
  std::unordered_set<int64_t> nograd;
  std::vector<SegPlan> plan;           // per backward segment
  bool grad_at(int64_t o) const { return nograd.empty() || !nograd.count(o); }
  bool w_grad(const LinearP& l) const {
    for (int k = 0; k < l.parts; ++k) if (grad_at(l.w + k * ((int64_t)l.in * l.out / l.parts))) return true;
    return false;
  }
  bool b_grad(const LinearP& l) const {
    for (int k = 0; k < l.parts; ++k) if (grad_at(l.b + k * (l.out / l.parts))) return true;
    return false;
  }
  // The Linear rule: the weight-gradient GEMM of a Linear inside a running step is left out only when its weight has no gradient and
  // no bias gradient rides on that GEMM (with_bias: QKV and FFN-up, whose bias sums come out of the GEMM's rowsum_out)
  bool drops_wgrad(const LinearP& l, bool with_bias) const { return !nograd.empty() && !w_grad(l) && !(with_bias && b_grad(l)); }
  std::vector<Tap> taps;
  std::vector<StepIn> in;            // in[i]: the hidden states schedule step i starts from; in[sched.size()]: the encoder's outputs
  int cur_t = 0, cur_v = 0;          // ping-pong index of the running activation gradients
  bool bad = false;
  int64_t P(const std::string& k) {
    auto it = off.find(k);
    if (it == off.end()) { crct_set_error("engine: parameter '%s' missing from the layout", k.c_str()); bad = true; return 0; }
    return it->second;
  }
};

// The attention (kind, index, direction) at token / visual lengths T / V; a triple that names none is refused with `who` in front of the
// message.  The only place that knows the co-attention's cross wiring (vilbert.py:684-723): text queries read the VISUAL keys and values
// (qkv1) under the image mask with p_v_attn at the layer's first dropout site, visual queries the TEXT ones (qkv2) under the text mask
// with p_attn at the site behind it.
int crct_engine::attn_site(const char* who, int kind, int index, int direction, int T, int V, AttnSite* out) const {
  AttnSite s;
  s.kind = kind; s.index = index; s.direction = direction;
  if (kind == 0 || kind == 1) {
    const std::vector<SelfLayerP>& lp = kind == 0 ? tl : vl;
    CRCT_REQUIRE(index >= 0 && index < (int)lp.size(), "%s: %s layer %d out of range [0,%d)", who, kind == 0 ? "text" : "visual", index, (int)lp.size());
    CRCT_REQUIRE(direction == 0, "%s: direction %d belongs to connection layers (kind 2)", who, direction);
    const SelfLayerP& p = lp[index];
    const SelfLayerA& a = (kind == 0 ? tla : vla)[index];
    s.heads = p.heads; s.d = p.H / p.heads; s.Tq = s.Tk = kind == 0 ? T : V; s.image_keys = kind == 1;
    s.q = s.k = a.qkv; s.p = p.p_attn; s.site = p.site;
    s.lse = a.lse; s.ctx = a.ctx; s.ctxq = a.ctxq; s.site_ctx = a.site_ctx;
  } else {
    CRCT_REQUIRE(kind == 2, "%s: unknown kind %d (0 text, 1 visual, 2 connection layer)", who, kind);
    const int layers = d.with_coattention ? (int)cl.size() : 0;
    CRCT_REQUIRE(index >= 0 && index < layers, "%s: connection layer %d out of range [0,%d)", who, index, layers);
    CRCT_REQUIRE(direction == 0 || direction == 1, "%s: direction %d must be 0 (text over visual) or 1 (visual over text)", who, direction);
    const ConnLayerA& a = cla[index];
    const bool tq = direction == 0;      // text queries
    s.heads = d.b_heads; s.d = d.Hb / d.b_heads; s.Tq = tq ? T : V; s.Tk = tq ? V : T; s.image_keys = tq;
    s.q = tq ? a.qkv2 : a.qkv1; s.k = tq ? a.qkv1 : a.qkv2; s.p = tq ? d.p_v_attn : d.p_attn; s.site = cl[index].site + (tq ? 0 : 1);
    s.lse = tq ? a.lse1 : a.lse2; s.ctx = tq ? a.ctx1 : a.ctx2; s.ctxq = tq ? a.ctx1q : a.ctx2q; s.site_ctx = tq ? a.site_ctx1 : a.site_ctx2;
  }
  s.k += (size_t)s.H() * sizeof(bf16_t);      // q | k | v side by side in a row of the key side's buffer
  s.v = s.k + (size_t)s.H() * sizeof(bf16_t); s.ld = 3 * (int64_t)s.H();
  *out = s;
  return 0;
}

namespace {

LinearP linear_p(crct_engine* e, const std::string& name, int in, int out, int site = CRCT_SITE_HEAD) {
  LinearP l;
  l.w = e->P(name + ".weight"); l.b = e->P(name + ".bias"); l.in = in; l.out = out; l.site = site;
  return l;
}
LnP ln_p(crct_engine* e, const std::string& name) {
  LnP l; l.g = e->P(name + ".weight"); l.b = e->P(name + ".bias"); return l;
}
// three Linear(in, out) stored back to back -> one Linear(in, 3*out)
LinearP fused3(crct_engine* e, const std::string& a, const std::string& b, const std::string& c, int in, int out, int site) {
  LinearP l = linear_p(e, a, in, 3 * out, site);
  l.parts = 3;
  const int64_t wsz = (int64_t)in * out;
  if (e->P(b + ".weight") != l.w + wsz || e->P(c + ".weight") != l.w + 2 * wsz || e->P(b + ".bias") != l.b + out ||
      e->P(c + ".bias") != l.b + 2 * out) {
    crct_set_error("engine: %s / %s / %s must be adjacent in the flat layout (fused QKV)", a.c_str(), b.c_str(), c.c_str());
    e->bad = true;
  }
  return l;
}

// A self-attention layer (BertLayer / BertImageLayer) from the prefix of its parameter names, its sizes and dropout probabilities,
// its first dropout site and the first of its four GEMM sites (QKV, OUT, FFN_UP, FFN_DN)
static_assert(CRCT_SITE_T_OUT == CRCT_SITE_T_QKV + 1 && CRCT_SITE_T_FFN_UP == CRCT_SITE_T_QKV + 2 && CRCT_SITE_T_FFN_DN == CRCT_SITE_T_QKV + 3 &&
              CRCT_SITE_V_OUT == CRCT_SITE_V_QKV + 1 && CRCT_SITE_V_FFN_UP == CRCT_SITE_V_QKV + 2 && CRCT_SITE_V_FFN_DN == CRCT_SITE_V_QKV + 3,
              "the GEMM sites of a self-attention layer are consecutive");
SelfLayerP self_layer_p(crct_engine* e, const std::string& p, int H, int I, int heads, float p_attn, float p_hid, uint32_t drop_site, int gemm_site) {
  SelfLayerP l;
  l.H = H; l.heads = heads; l.p_attn = p_attn; l.p_hid = p_hid; l.site = drop_site;
  l.qkv = fused3(e, p + "attention.self.query", p + "attention.self.key", p + "attention.self.value", H, H, gemm_site);
  l.proj.dense = linear_p(e, p + "attention.output.dense", H, H, gemm_site + 1);
  l.proj.ln = ln_p(e, p + "attention.output.LayerNorm");
  l.ffn.up = linear_p(e, p + "intermediate.dense", H, I, gemm_site + 2);
  l.ffn.down = linear_p(e, p + "output.dense", I, H, gemm_site + 3);
  l.ffn.ln = ln_p(e, p + "output.LayerNorm");
  return l;
}
// every Linear of the encoder layers, in the order their fp8 scale slots are numbered
template <class F> void each_encoder_linear(const crct_engine* e, F f) {
  for (const std::vector<SelfLayerP>* stack : {&e->tl, &e->vl})
    for (const SelfLayerP& l : *stack) { f(l.qkv); f(l.ffn.up); f(l.ffn.down); f(l.proj.dense); }
  for (const ConnLayerP& l : e->cl) {
    f(l.qkv1); f(l.qkv2); f(l.ffn_v.up); f(l.ffn_v.down); f(l.ffn_t.up); f(l.ffn_t.down); f(l.proj_v.dense); f(l.proj_t.dense);
  }
}

FfnA ffn_a(Arena& ar, size_t M, int H, int I, int& sites, int& gsites) {
  FfnA a;
  a.g_dl = gsites++; a.g_du = gsites++;
  a.u = ar.take(M * I * 2); a.h = ar.take(M * I * 2); a.s = ar.take(M * H * 4); a.y = ar.take(M * H * 2); a.y32 = NONE;
  a.mean = ar.take(M * 4); a.rstd = ar.take(M * 4);
  a.hq = ar.take(M * I); a.yq = ar.take(M * H);
  a.site_h = sites++; a.site_y = sites++;
  return a;
}
ProjA proj_a(Arena& ar, size_t M, int H, int& sites, int& gsites) {
  ProjA a;
  a.g_dl = gsites++;
  a.s = ar.take(M * H * 4); a.a = ar.take(M * H * 2); a.a32 = NONE; a.mean = ar.take(M * 4); a.rstd = ar.take(M * 4);
  a.aq = ar.take(M * H);
  a.site_a = sites++;
  return a;
}
// the activations of a self-attention layer over M rows (the order of the takes and of the site numbers is the workspace's layout)
SelfLayerA self_layer_a(Arena& ar, size_t M, int H, int I, int heads, int& sites, int& gsites) {
  SelfLayerA a;
  a.qkv = ar.take(M * 3 * H * 2); a.ctx = ar.take(M * H * 2); a.ctxq = ar.take(M * H); a.lse = ar.take(M * heads * 4);
  a.site_ctx = sites++; a.g_dqkv = gsites++;
  a.proj = proj_a(ar, M, H, sites, gsites); a.ffn = ffn_a(ar, M, H, I, sites, gsites);
  return a;
}
StreamScratch scratch_a(Arena& ar, size_t M, int H, int I, int Hb) {
  StreamScratch s;
  const int Hm = H > Hb ? H : Hb;
  s.dy[0] = ar.take(M * H * 2); s.dy[1] = ar.take(M * H * 2);
  s.dres_a = ar.take(M * H * 2); s.dlin_a = ar.take(M * H * 2); s.dres_b = ar.take(M * H * 2); s.dlin_b = ar.take(M * H * 2);
  s.gc = ar.take(M * H * 2); s.du = ar.take(M * (size_t)I * 2); s.dctx = ar.take(M * (size_t)Hm * 2);
  s.dqkv = ar.take(M * (size_t)3 * Hm * 2);
  s.part_a = ar.take((size_t)3 * 4 * CRCT_LN_BWD_MAX_BLOCKS * H * 4);   // [3][4 waves x blocks][H]      // LayerNorm-backward column partials of the layer's two norms
  s.part_b = ar.take((size_t)3 * 4 * CRCT_LN_BWD_MAX_BLOCKS * H * 4);
  s.dlq_a = ar.take(M * H); s.dlq_b = ar.take(M * H); s.duq = ar.take(M * (size_t)I);
  s.dqkvq = ar.take(M * (size_t)3 * Hm);
  return s;
}

// ================================================================================ per-call context
hipEvent_t ev_new(crct_engine* e) {
  if (e->evnext == e->evpool.size()) {
    hipEvent_t ev = nullptr;
    // ordering between streams of ONE device: no system-scope fence (host / peer visibility) at the record -- the hand-off
    // is 2.5-4 us shorter (tools/handoff_lab.cpp)
    const unsigned flags = hipEventDisableTiming | hipEventDisableSystemFence;
    if (hipEventCreateWithFlags(&ev, flags) != hipSuccess) return nullptr;
    e->evpool.push_back(ev);
  }
  return e->evpool[e->evnext++];
}
// everything enqueued on `from` so far happens before whatever is enqueued on `to` from now on
int order_streams(crct_engine* e, hipStream_t from, hipStream_t to) {
  if (from == to) return 0;
  hipEvent_t ev = ev_new(e);
  if (!ev || hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess) {
    crct_set_error("engine: event ordering between internal streams failed");
    return 1;
  }
  return 0;
}

// fp8 copies of a weight gradient's operands (Run::lin_wgrad): the e5m2 copy of dy, the e4m3 copy of x
struct WgQ8 { GradQ dy; Act x; };
// an fp8 tensor of the workspace with its scale and amax words, as pointers (q == nullptr: none)
struct Q8 { uint8_t* q = nullptr; const float* scale = nullptr; float* amax = nullptr; };

struct Run {
  crct_engine* e;
  const float* p32; const bf16_t* p16; float* g32; char* ws; hipStream_t s;
  const CrctBatch* b; const CrctStepCfg* c;
  hipStream_t sw;                      // stream of this data stream's weight-gradient GEMMs (== s when disabled)
  size_t partials, colsum_part, colsum_part_w;
  int which = 0;                       // 0 = text stream, 1 = visual stream (owner of split-K workspace `which`)
  int phase = 1;                       // 0: text-only part of the schedule, 1: beside the visual stream (site policy)
  int rc = 0;
  bool sw_dirty = false;               // sw has work that s has not been ordered after yet (no empty forks / joins)
  // scratch double-buffering: layer n of this data stream uses scratch set (n & 1); before reusing a set the
  // data stream waits only for the weight-gradient work of the layer that used it LAST (two layers ago)
  const StreamScratch* sets[2] = {nullptr, nullptr};
  hipEvent_t set_free[2] = {nullptr, nullptr};
  int parity = 0;
  const StreamScratch& layer_begin() {
    if (!rc && sw != s && set_free[parity]) {
      if (hipStreamWaitEvent(s, set_free[parity], 0) != hipSuccess) { crct_set_error("engine: stream wait failed"); rc = 1; }
      set_free[parity] = nullptr;
    }
    return *sets[parity];
  }
  void layer_end() {
    flush_wgrads();
    if (!rc && sw != s && sw_dirty) {
      hipEvent_t ev = ev_new(e);
      if (!ev || hipEventRecord(ev, sw) != hipSuccess) { crct_set_error("engine: event record failed"); rc = 1; }
      set_free[parity] = ev;
    }
    parity ^= 1;
  }
  std::vector<CrctGemmArgs> pending;   // weight-gradient GEMMs of the current layer, launched as ONE grouped grid
  bool defer_wgrad = true;             // false: launch every weight gradient immediately on s (buffers are recycled)
  struct FinJob { const float* part; float* dg; float* db; float* dlb; int M, H; };
  std::vector<FinJob> pending_fin;     // LayerNorm column passes of the current layer (run on sw at the layer's flush)
  int tick = 0, ordered_tick = -1;     // launches enqueued on s / the tick sw was last ordered after (skip redundant events)
  void wgrad_after_main() {            // sw sees what s produced
    if (rc || sw == s) return;
    sw_dirty = true;
    if (ordered_tick == tick) return;  // nothing new on s since the last ordering: sw is already behind it
    fail(order_streams(e, s, sw));
    ordered_tick = tick;
  }
  void main_after_wgrad() {            // s may overwrite what sw read
    flush_wgrads();
    if (!rc && sw != s && sw_dirty) { fail(order_streams(e, sw, s)); sw_dirty = false; }
  }

  template <class T> T* W(size_t o) const { return reinterpret_cast<T*>(ws + o); }
  bf16_t* A(size_t o) const { return W<bf16_t>(o); }
  float* F(size_t o) const { return W<float>(o); }
  const float* P(int64_t o) const { return p32 + o; }
  const bf16_t* PB(int64_t o) const { return p16 + o; }
  float* G(int64_t o) const { return g32 + o; }
  Drop drop(float p, uint32_t site) const { return drop_of(c, p, site); }
  void fail(int r) { if (!rc && r) rc = r; }
  AttnSite site(int kind, int index, int direction) {      // an attention of the running batch (schedule indices: never refused)
    AttnSite a;
    fail(e->attn_site("engine", kind, index, direction, b->T, b->V, &a));
    return a;
  }
  const uint8_t* keymask(const AttnSite& a) const { return a.image_keys ? b->image_keymask : b->text_keymask; }

  struct Opt {
    void* preact = nullptr; const void* dact_src = nullptr; int dact = 0; int act = 0;
    const void* addend = nullptr; int64_t ld_aux = 0, ld_add = 0; Drop drop; bool f32 = false; bool acc = false;
    bool add_f32 = false, c_cached = false;      // the fp32 residual stream: fp32 addend; fp32 output that the next kernel reads
    CrctGemmLnAddend ln = {nullptr, nullptr, nullptr, nullptr};      // ... the addend is the LayerNorm of those fp32 rows (forward only)
  };
  // both sides reach this point before either goes on: the two data streams are ordered against each other
  void cross_sync(Run& V) {
    if (!rc) fail(order_streams(e, V.s, s));
    if (!V.rc) V.fail(order_streams(e, s, V.s));
  }
  // ---- fp8 forward (CrctStepCfg.fp8): a Linear reads the e4m3 copies of its input and of its weight; optionally it also emits the
  // e4m3 copy of its own output for the next fp8 GEMM
  // CrctStepCfg.fp8 == 2 (calibration, the dry pass before the first fp8 forward): every producer writes its copy and collects its
  // maximum, the GEMMs themselves still read the bf16 operands -- the maxima are then those of the bf16 forward, not of a forward
  // whose GEMMs ran on unscaled (scale 1) e4m3 inputs
  int f8() const { return (c->fp8 && c->params_fp8 && c->fp8_w_scale && c->fp8_act_scale && c->fp8_act_amax) ? c->fp8 : 0; }
  bool f8_lin(const LinearP& l) const { return f8() && e->wq_slot.count(l.w) != 0; }
  // ---- fp8 backward (CrctStepCfg.fp8_bwd): data gradients dx = dy W of the FFN and attention-output Linears from the e5m2 copy
  // of dy (written by the producing LayerNorm-backward / GELU' epilogue / attention backward) and the TRANSPOSED e4m3 weight shadow.
  // fp8_bwd == 2 (calibration, the first backward pass): the producers collect the gradient maxima, the GEMMs still run in bf16.
  int f8b() const { return (c->fp8 && c->fp8_bwd && c->params_fp8_t && c->fp8_w_scale && c->fp8_grad_scale && c->fp8_grad_amax) ? c->fp8_bwd : 0; }
  bool f8b_lin(const LinearP& l) const { return f8b() && e->wq_slot.count(l.w) != 0; }
  // scale and amax words of an activation / gradient scale site
  const float* ascale(int site) const { return c->fp8_act_scale + site; }
  float* aamax(int site) const { return c->fp8_act_amax + (int64_t)site * CRCT_FP8_AMAX_LANES; }
  const float* gscale(int g) const { return c->fp8_grad_scale + g; }
  float* gamax(int g) const { return c->fp8_grad_amax + (int64_t)g * CRCT_FP8_AMAX_LANES; }
  Q8 q8(const Act& a) const { return a.site < 0 ? Q8() : Q8{W<uint8_t>(a.q), ascale(a.site), aamax(a.site)}; }
  Q8 q8(const GradQ& g) const { return g.site < 0 ? Q8() : Q8{W<uint8_t>(g.q), gscale(g.site), gamax(g.site)}; }

  enum Dir { FWD = CRCT_KIND_FWD, DGRAD = CRCT_KIND_DGRAD, WGRAD = CRCT_KIND_WGRAD };
  // The one place a CrctGemmArgs is filled in: the three GEMMs of Linear l over M rows.
  //   FWD    C[M][out] = a[M][in] W^T + b      DGRAD  C[M][in] = a[M][out] W      WGRAD  C[out][in] = a[M][out]^T x[M][in]
  // (x is read by WGRAD only).  a8: the fp8 copy of `a` -- when given the GEMM runs on fp8 operands, against the e4m3 weight shadow
  // (FWD), its transpose (DGRAD) or x8, the e4m3 copy of x (WGRAD).  out: where to leave an fp8 copy of the result and its maximum
  // (e4m3 of a forward result, e5m2 of a gradient) -- also behind bf16 operands, which is what the calibration passes run.
  // The site's launch policy: its configuration for every kind; split-K only for the bf16 forward / data-gradient GEMMs (all of them
  // run on the data stream, whose split-K workspace `which` this Run owns).
  CrctGemmArgs gemm_args(Dir dir, const LinearP& l, int M, const void* a, int64_t lda, const void* x, int64_t ldx, void* C, int64_t ldc,
                         const Opt& o, const Q8& a8 = Q8(), const Q8& x8 = Q8(), const Q8& out = Q8()) const {
    const bool q = a8.q != nullptr;
    CrctGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = q ? a8.q : a; g.C = C; g.ldc = ldc;
    if (dir == WGRAD) {
      g.B = q ? x8.q : x; g.M = l.out; g.N = l.in; g.K = M; g.ta = 1; g.tb = 1; g.lda = lda; g.ldb = ldx;
    } else {
      const bool fwd = dir == FWD;
      g.M = M; g.N = fwd ? l.out : l.in; g.K = fwd ? l.in : l.out;
      // the fp8 copies are dense, and the transposed shadow is K-contiguous for the data gradient as the weight is for the forward
      g.lda = q ? g.K : lda; g.ldb = q ? g.K : l.in; g.tb = !fwd && !q;
      if (q) g.B = reinterpret_cast<const uint8_t*>(fwd ? c->params_fp8 : c->params_fp8_t) + l.w;
      else g.B = PB(l.w);
      if (fwd) g.bias = P(l.b);
    }
    g.preact_out = o.preact; g.dact_src = o.dact_src; g.addend = o.addend; g.ld_aux = o.ld_aux; g.ld_add = o.ld_add;
    g.act = o.act; g.dact = o.dact; g.c_is_f32 = o.f32; g.accumulate = o.acc; g.addend_f32 = o.add_f32; g.c_cached = o.c_cached;
    g.alpha = 1.0f; g.drop_thr = o.drop.thr; g.drop_scale = o.drop.scale; g.drop_site = o.drop.site; g.seed = c->seed; g.site = l.site;
    if (q) {
      // bit 0: fp8 operands, bit 1: A is an e5m2 gradient, bit 3: labelled as a data gradient (no transposed B tells it apart)
      g.fp8 = dir == FWD ? 1 : (dir == DGRAD ? 1 | 2 | 8 : 1 | 2);
      g.scale_a = a8.scale; g.scale_b = dir == WGRAD ? x8.scale : c->fp8_w_scale + e->wq_slot.at(l.w);
    }
    if (out.q) {
      g.q_out = out.q; g.q_scale = out.scale; g.q_amax = out.amax; g.ld_q = g.N;
      if (dir == DGRAD) g.fp8 |= 4;                       // bit 2: the copy is e5m2 (a gradient), not e4m3 (an activation)
    }
    g.tile = -1;
    if (l.site > 0 && l.site < CRCT_SITE_COUNT) {
      const crct_engine::SitePolicy& pol = e->policy[l.site][dir][phase];
      if (pol.cfg >= 0) g.tile = pol.cfg;
      if (dir != WGRAD && !q && pol.split_k > 1 && crct_gemm_splitk_ws_elems(g.M, g.N, pol.split_k) <= (int64_t)e->sk_ws_elems[which] &&
          crct_gemm_splitk_tickets(g.M, g.N) <= e->sk_tickets) {
        g.split_k = pol.split_k; g.splitk_ws = F(e->sk_ws[which]); g.splitk_cnt = W<uint32_t>(e->sk_cnt[which]);
      }
    }
    return g;
  }
  void launch(const CrctGemmArgs& g, const CrctGemmLnAddend* ln = nullptr) {      // on the data stream: one tick per launch
    ++tick;
    fail(crct_gemm_bf16_ln_addend(&g, ln && ln->mean ? ln : nullptr, s));
  }

  // y[M][out] = x W^T + b (+ epilogue), in the precision the Linear itself decides.  The forward rules, all of them:
  //  * fp8 operands iff the weight has an e4m3 shadow in an fp8 forward (f8_lin) AND the input comes with an e4m3 copy
  //    (x.site >= 0).  Every hidden state and every attention-output LayerNorm's result has one (ln_fwd, the embeddings); the
  //    attention context only where the attention kernel wrote it (ctx_act: attn_q_ok); the FFN's h only when the up projection
  //    qualified and the down projection is fp8-capable (ffn_h) -- the returned Act says so.
  //  * y.site >= 0 asks for the e4m3 copy and maximum of the result; only a Linear that qualifies for fp8 writes them.
  //  * calibration (f8() == 2): the GEMM reads the bf16 operands and still writes the copy and maximum it was asked for.
  // Returns y, with site -1 where no copy was written.
  Act lin_fwd(const Act& x, int64_t ldx, const LinearP& l, int M, Act y, int64_t ldy, const Opt& o) {
    const bool q = f8_lin(l) && x.site >= 0;
    if (!q) y.site = -1;
    if (rc) return y;
    launch(gemm_args(FWD, l, M, A(x.x), ldx, nullptr, 0, A(y.x), ldy, o, q && f8() == 1 ? q8(x) : Q8(), Q8(), q8(y)), &o.ln);
    return y;
  }
  // dx[M][in] = dy W (+ epilogue).  The data-gradient rules:
  //  * fp8 operands iff the weight has a transposed e4m3 shadow in an fp8 backward (f8b_lin) AND dy comes with an e5m2 copy
  //    (dyq.site >= 0): the LayerNorm backward writes one for an fp8-backward-capable Linear (ln_bwd), the FFN-down data gradient
  //    for an fp8-backward-capable up projection (ffn_bwd), the attention backward for QKV projections that also ran their forward
  //    in fp8 (self_bwd / conn_bwd: the weight gradient reads the same copy against the layer input's e4m3 copy).
  //  * out.site >= 0 asks for the e5m2 copy and maximum of dx; only a Linear that qualifies writes them.
  //  * calibration (f8b() != 1): the GEMM reads the bf16 operands and still writes the copy and maximum it was asked for.
  // Returns `out`, with site -1 where no copy was written.
  GradQ lin_dgrad(const void* dy, int64_t lddy, const LinearP& l, int M, void* dx, int64_t lddx, const Opt& o, const GradQ& dyq = GradQ(),
                  GradQ out = GradQ()) {
    const bool q = f8b_lin(l) && dyq.site >= 0;
    if (!q) out.site = -1;
    if (rc) return out;
    launch(gemm_args(DGRAD, l, M, dy, lddy, nullptr, 0, dx, lddx, o, q && f8b() == 1 ? q8(dyq) : Q8(), Q8(), q8(out)));
    return out;
  }
  // dW[out][in] += dy^T x
  // with_bias: also db[out] += column sums of dy.  When the contraction length qualifies for the LDS-DMA kernel the
  // sums come out of the weight-gradient kernel itself (CrctGemmArgs.rowsum_out); otherwise a column-sum launch.
  // w8: the fp8 copies of both operands where the other passes left them (fp8 backward, CrctStepCfg.fp8_wgrad): dy as OCP e5m2
  // with its gradient scale site, x as e4m3 with its activation scale site -- x's copy is only there behind an fp8 forward of this
  // Linear (f8_lin).  The weight gradient then reads half the bytes (gemm.hip, fp8 weight gradients); the bias gradient still sums
  // the bf16 dy.
  void lin_wgrad(const void* dy, int64_t lddy, const void* x, int64_t ldx, const LinearP& l, int M, bool with_bias = false, const WgQ8& w8 = WgQ8()) {
    if (rc) return;
    const bool keep = !e->drops_wgrad(l, with_bias);      // a dropped GEMM keeps its place in the layer's group (flush_wgrads)
    if (!keep && !defer_wgrad) return;
    const bool f8w = f8b() == 1 && c->fp8_wgrad && defer_wgrad && f8_lin(l) && w8.dy.site >= 0 && w8.x.site >= 0 &&
                     l.in % 16 == 0 && l.out % 16 == 0 && lddy % 16 == 0 && ldx % 16 == 0;
    const bool fold = !f8w && with_bias && M % 64 == 0 && l.in % 8 == 0 && l.out % 8 == 0 && lddy % 8 == 0 && ldx % 8 == 0;
    if (with_bias && !fold && keep) bias_grad(dy, lddy, l, M);
    if (rc) return;
    Opt o; o.f32 = true; o.acc = true;
    CrctGemmArgs g = gemm_args(WGRAD, l, M, dy, lddy, x, ldx, G(l.w), l.in, o, f8w ? q8(w8.dy) : Q8(), f8w ? q8(w8.x) : Q8());
    if (keep && c->wgrad_overwrite && e->wgrad_owned.count(l.w)) {
      if (++e->wgrad_pass[l.w] > 1) { rc = 1; crct_set_error("engine_backward: weight gradient at offset %lld is produced twice in one pass but is listed as owned", (long long)l.w); return; }
      g.accumulate = 0;               // the only producer of this gradient: write it, whatever the buffer held
      if (c->grads_bf16) {            // ... straight into the exchange's bf16 buffer (CrctStepCfg.grads_bf16): the caller packs none of the owned gradients
        if (l.in % 8 != 0 || l.w % 8 != 0) { rc = 1; crct_set_error("engine_backward: owned weight gradient at offset %lld (in = %d) cannot be written as bf16 rows", (long long)l.w, l.in); return; }
        g.C = reinterpret_cast<bf16_t*>(c->grads_bf16) + l.w; g.c_is_f32 = 0;
      }
    }
    if (fold) g.rowsum_out = G(l.b);
    if (f8w) {
      if (!keep) return;                                  // (a weight with an e4m3 shadow and no gradient is refused by the caller)
      g.tile = crct_gemm_fp8_wgrad_step_config(g.tile);   // 2 stages (two workgroups per CU) unless the site policy asks for 3
      pending_f8.push_back(g);
      return;
    }
    if (!defer_wgrad) { launch(g); return; }              // head chain: in order, right now
    // queued also without a side stream (sw == s): the same groups, hence the same kernels and summation orders,
    // in every stream mode -- results stay bit-identical across modes
    pending.push_back(g);
    pending_keep.push_back(keep);
    if (pending.size() == 8) flush_wgrads();
  }
  // launch the queued weight-gradient GEMMs on the side stream, ordered after everything enqueued on s so far
  std::vector<CrctGemmArgs> pending_f8;      // the layer's fp8 weight gradients: one grouped launch of their own
  // pending[i] is launched iff pending_keep[i]: a GEMM the Linear rule drops stays in the list, so that the groups are cut at the
  // same places and take the configuration and the kernel they would have had with it (CrctGemmGroup.keep)
  std::vector<uint8_t> pending_keep;
  void flush_wgrads() {
    if (!pending.empty() && std::find(pending_keep.begin(), pending_keep.end(), 1) == pending_keep.end()) { pending.clear(); pending_keep.clear(); }
    if (rc || (pending.empty() && pending_f8.empty() && pending_fin.empty() && pending_bias.empty())) return;
    if (sw == s) ++tick;
    wgrad_after_main();
    for (const BiasJob& j : pending_bias)
      if (!rc) fail(crct_colsum_bf16(j.dy, j.lddy, j.db, F(sw != s ? colsum_part_w : colsum_part), j.M, j.N, 1, sw));
    pending_bias.clear();
    for (const FinJob& f : pending_fin)
      if (!rc) fail(crct_layernorm_bwd_finalize(f.part, f.dg, f.db, f.dlb, f.M, f.H, 1, sw));
    pending_fin.clear();
    // a persistent grid for the group (gemm.hip, group_grid) where the throttled side stream stays off the critical path: a side
    // stream per data stream, and not the 2560 / 6400-row streams of the long-context configuration, whose data-gradient GEMMs fill the
    // chip themselves (measured there: 11.90 - 11.94 ms with the text stream's groups throttled, 11.96 - 12.04 with both, 11.80 - 11.86 without)
    // (not on the exchange mode's shared side stream, which would become the critical path: 8.0 -> 8.9 - 9.1 ms at 96 workgroups)
    const int target = (sw != s && !pending.empty() && pending[0].K <= e->wgrad_target_rows && !e->one_wgrad_stream) ? e->wgrad_target : 0;
    for (size_t i = 0; i < pending.size() && !rc; i += 8) {
      const int ng = (int)std::min<size_t>(8, pending.size() - i);
      const uint8_t* kp = pending_keep.data() + i;
      fail(gemm_grouped_checked(CrctGemmGroup{pending.data() + i, nullptr, ng, std::find(kp, kp + ng, 0) == kp + ng ? nullptr : kp, target}, sw));
    }
    pending.clear();
    pending_keep.clear();
    for (size_t i = 0; i < pending_f8.size() && !rc; i += 8)
      fail(crct_gemm_bf16_grouped(pending_f8.data() + i, (int)std::min<size_t>(8, pending_f8.size() - i), sw));
    pending_f8.clear();
  }
  // db[out] += column sums of dy: queued like the weight gradients (dy stays valid until the layer's flush), so the data
  // stream carries no ordering event per call -- the head chain alone had 13 of them between its 13 small data-gradient GEMMs
  struct BiasJob { const void* dy; int64_t lddy; float* db; int M, N; };
  std::vector<BiasJob> pending_bias;
  void bias_grad(const void* dy, int64_t lddy, const LinearP& l, int M) {
    if (rc) return;
    if (defer_wgrad) { pending_bias.push_back(BiasJob{dy, lddy, G(l.b), M, l.out}); return; }
    wgrad_after_main();
    if (rc) return;
    fail(crct_colsum_bf16(dy, lddy, G(l.b), F(sw != s ? colsum_part_w : colsum_part), M, l.out, 1, sw));
  }
  // y: the LayerNorm's output with its e4m3 and fp32 copies (ProjA::out / FfnA::out)
  void ln_fwd(size_t x, const LnP& ln, const Act& y, size_t mean, size_t rstd, int M, int H) {
    if (rc) return;
    ++tick;
    CrctLnFwdArgs a = {A(x), P(ln.g), P(ln.b), A(y.x), F(mean), F(rstd), M, H, 1e-12f, 0, 1.f, 0, c->seed, nullptr, nullptr, nullptr, 0, nullptr};
    if (r32()) { a.x_f32 = 1; if (!e->ln_addend) a.y_f32 = F(y.x32); }
    if (f8()) { a.q_out = W<uint8_t>(y.q); a.q_scale = ascale(y.site); a.q_amax = aamax(y.site); }
    fail(crct_layernorm_fwd_args(&a, s));
  }
  // The fp32 residual stream (CrctStepCfg.residual_fp32): the pre-LayerNorm sums are written and read as fp32, and every block adds
  // the fp32 value of its input where a LayerNorm produced it (the embeddings' outputs have none: bf16 there, one rounding).  The
  // closing GEMM's epilogue rebuilds that value from the LayerNorm's own inputs -- s, which it reads instead of a copy (the same 4
  // bytes per element), two floats per row and two per column -- so the LayerNorm stores its bf16 output only; the rows, statistics
  // and parameters all outlive the block (the backward pass reads them; no buffer of the plan is recycled within a forward, evaluation
  // included).  ln_addend == 0: the LayerNorm writes the fp32 copy x32 and the epilogue adds that (same bits).
  bool r32() const { return c->residual_fp32 != 0; }
  void residual(Opt& o, const Act& x, int64_t ld) const {
    o.ld_add = ld;
    if (r32()) {
      o.f32 = true; o.c_cached = true;
      if (e->ln_addend && x.s != NONE) {
        o.addend = F(x.s); o.add_f32 = true;
        o.ln = CrctGemmLnAddend{F(x.mean), F(x.rstd), P(x.ln.g), P(x.ln.b)};
        return;
      }
      if (!e->ln_addend && x.x32 != NONE) { o.addend = F(x.x32); o.add_f32 = true; return; }
    }
    o.addend = A(x.x);
  }
  // returns the buffer that holds the gradient of the producing Linear's output; dlq: where its e5m2 copy may go -- written for an
  // fp8-backward-capable Linear, site -1 on return otherwise
  size_t ln_bwd(size_t dy, size_t x, size_t mean, size_t rstd, const LnP& ln, const LinearP& lin, size_t dres, size_t dlin,
                size_t part, int M, int H, const Drop& dr, GradQ& dlq) {
    if (!f8b_lin(lin)) dlq.site = -1;
    if (rc) return dres;
    // rows pass on the data stream; the column pass (dgamma, dbeta, bias gradient of the producing Linear) joins the
    // weight-gradient work on the side stream -- `part` belongs to this layer's scratch set
    ++tick;
    CrctLnBwdArgs a = {A(dy), A(x), F(mean), F(rstd), P(ln.g), A(dres), dr.thr ? A(dlin) : nullptr, F(part), M, H,
                       0, 1.f, 0, dr.thr, dr.scale, dr.site, c->seed, nullptr, nullptr, nullptr, r32() ? 1 : 0};
    if (dlq.site >= 0) { const Q8 d8 = q8(dlq); a.q_out = d8.q; a.q_scale = d8.scale; a.q_amax = d8.amax; }
    fail(crct_layernorm_bwd_rows_args(&a, s));
    // the column pass is queued like the weight gradients: ONE ordering event per layer covers all of them
    if (defer_wgrad) pending_fin.push_back(FinJob{F(part), G(ln.g), G(ln.b), G(lin.b), M, H});
    else { wgrad_after_main(); if (!rc) fail(crct_layernorm_bwd_finalize(F(part), G(ln.g), G(ln.b), G(lin.b), M, H, 1, sw)); }
    return dr.thr ? dlin : dres;
  }
  // ctx.site >= 0: also the e4m3 copy of ctx (the fp8 forward GEMM and weight gradient of the attention-output projection read it)
  void attn_fwd(const AttnSite& a, const Act& ctx) {
    if (rc) return;
    ++tick;
    const Drop dr = drop(a.p, a.site);
    CrctAttnQuant qz;
    memset(&qz, 0, sizeof(qz));
    qz.row_lse = F(a.lse);
    if (ctx.site >= 0) { const Q8 c8 = q8(ctx); qz.ctx_q = c8.q; qz.ctx_scale = c8.scale; qz.ctx_amax = c8.amax; }
    fail(crct_attention_fwd_q(A(a.q), A(a.k), A(a.v), keymask(a), A(ctx.x), b->B, a.heads, a.Tq, a.Tk, a.d, a.ld, a.ld, a.ld, a.H(), dr.thr,
                              dr.scale, dr.site, c->seed, &qz, s));
  }
  // dq goes to the query columns of the fused dqkv buffer at dqkv_q, dk / dv to the key and value columns of the one at dqkv_kv (the other
  // stream's in a co-attention); qq / kvq: the e5m2 copies of those buffers (one gradient scale site each), written where site >= 0
  void attn_bwd(const AttnSite& a, size_t dctx, size_t dqkv_q, size_t dqkv_kv, const GradQ& qq, const GradQ& kvq) {
    if (rc) return;
    ++tick;
    const Drop dr = drop(a.p, a.site);
    const int H = a.H();
    CrctAttnQuant qz;
    memset(&qz, 0, sizeof(qz));
    qz.row_lse = F(a.lse); qz.ctx = A(a.ctx); qz.ld_ctx = H;
    if (qq.site >= 0) { const Q8 d8 = q8(qq); qz.dq_q = d8.q; qz.dq_scale = d8.scale; qz.dq_amax = d8.amax; }
    if (kvq.site >= 0) { const Q8 d8 = q8(kvq); qz.dk_q = d8.q + H; qz.dv_q = d8.q + 2 * H; qz.dkv_scale = d8.scale; qz.dkv_amax = d8.amax; }
    fail(crct_attention_bwd_q(A(a.q), A(a.k), A(a.v), keymask(a), A(dctx), A(dqkv_q), A(dqkv_kv) + H, A(dqkv_kv) + 2 * H, b->B, a.heads, a.Tq, a.Tk,
                              a.d, a.ld, a.ld, a.ld, H, a.ld, a.ld, a.ld, dr.thr, dr.scale, dr.site, c->seed, &qz, s));
  }
  // The requested maps of one attention (crct_engine_set_attention_map_grads), right behind its attn_bwd on this stream: each adds its
  // contribution onto the dq / dk columns that launch wrote (same q, k, key mask and dropout stream; c = the step's gradient scale).
  // No request: nothing is launched and `tick` stays as it is
  void attn_map_grads(const AttnSite& a, size_t dqkv_q, size_t dqkv_kv) {
    for (const CrctAttnMapGrad& r : e->req.amg) {
      if (rc) return;
      if (r.kind != a.kind || r.index != a.index || r.direction != a.direction) continue;
      ++tick;
      const Drop dr = drop(a.p, a.site);
      fail(crct_attention_probs_bwd(A(a.q), A(a.k), keymask(a), r.d_probs, c->grad_scale, A(dqkv_q), A(dqkv_kv) + a.H(),
                                    F(e->req.amg_scratch(e->ws_base(), which)), 1, b->B, a.heads, a.Tq, a.Tk, a.d, a.ld, a.ld, a.ld, a.ld, dr.thr,
                                    dr.scale, dr.site, c->seed, s));
    }
  }
  // the attention kernels that write fp8 copies cover this shape (MFMA kernels: include/crct_hip.h, CrctAttnQuant)
  static bool attn_q_ok(const AttnSite& a) { return crct_attention_quant_ok(a.Tq, a.Tk, a.d) != 0; }
  // The attention context as both passes see it: its e4m3 copy exists where the attention kernel covers the shape (aq) and the
  // output projection `dense` runs its forward in fp8
  Act ctx_act(const AttnSite& a, const LinearP& dense, bool aq) const { return {a.ctx, a.ctxq, aq && f8_lin(dense) ? a.site_ctx : -1}; }
  // The FFN's hidden activation as both passes see it: hq exists when both forward GEMMs run in fp8
  Act ffn_h(const FfnP& p, const FfnA& a) const { return {a.h, a.hq, f8_lin(p.up) && f8_lin(p.down) ? a.site_h : -1}; }

  // ---------------------------------------------------------------- sub-blocks
  // a = LN(dropout(dense(ctx)) + x)          vilbert.py:424-428 / :555-559 / :749-756
  void proj_fwd(const ProjP& p, const ProjA& a, const Act& ctx, const Act& x, int M, const Drop& dr) {
    Opt o; o.drop = dr; residual(o, x, p.dense.out);
    lin_fwd(ctx, p.dense.in, p.dense, M, Act{a.s}, p.dense.out, o);
    ln_fwd(a.s, p.ln, a.out(p.ln), a.mean, a.rstd, M, p.dense.out);
  }
  // in: g = grad of a.  out: sc.dres_b (residual gradient), sc.dctx.  Parameter gradients accumulated.
  void proj_bwd(const ProjP& p, const ProjA& a, const Act& ctx, size_t g, const StreamScratch& sc, int M, const Drop& dr) {
    GradQ dlq{sc.dlq_b, a.g_dl};
    const size_t dl = ln_bwd(g, a.s, a.mean, a.rstd, p.ln, p.dense, sc.dres_b, sc.dlin_b, sc.part_b, M, p.dense.out, dr, dlq);
    lin_wgrad(A(dl), p.dense.out, A(ctx.x), p.dense.in, p.dense, M, false, WgQ8{dlq, ctx});
    lin_dgrad(A(dl), p.dense.out, p.dense, M, A(sc.dctx), p.dense.in, Opt(), dlq);
    if (e->wgrad_flush & 2) flush_wgrads();      // bit 1: the projection's weight gradient leaves behind its data gradient
  }
  // y = LN(dropout(down(gelu(up(x)))) + x)   vilbert.py:454-471 / :585-602 / :782-786
  void ffn_fwd(const FfnP& p, const FfnA& a, const Act& x, int M, const Drop& dr) {
    Opt o; o.preact = A(a.u); o.ld_aux = p.up.out; o.act = ACT_GELU;
    const Act h = lin_fwd(x, p.up.in, p.up, M, ffn_h(p, a), p.up.out, o);
    Opt o2; o2.drop = dr; residual(o2, x, p.down.out);
    lin_fwd(h, p.down.in, p.down, M, Act{a.s}, p.down.out, o2);
    ln_fwd(a.s, p.ln, a.out(p.ln), a.mean, a.rstd, M, p.down.out);
  }
  // in: g = grad of a.y.  out: gx = grad of x (the block's input: its e4m3 copy serves the fp8 weight gradient of the up projection).
  void ffn_bwd(const FfnP& p, const FfnA& a, const Act& x, size_t g, size_t gx, const StreamScratch& sc, int M, const Drop& dr) {
    const int H = p.down.out, I = p.up.out;
    GradQ dlq{sc.dlq_a, a.g_dl};
    const size_t dl = ln_bwd(g, a.s, a.mean, a.rstd, p.ln, p.down, sc.dres_a, sc.dlin_a, sc.part_a, M, H, dr, dlq);
    lin_wgrad(A(dl), H, A(a.h), I, p.down, M, false, WgQ8{dlq, ffn_h(p, a)});
    Opt o; o.dact_src = A(a.u); o.dact = ACT_GELU; o.ld_aux = I;
    // the e5m2 copy of du is asked for where the up projection's data gradient can read it
    const GradQ duq = lin_dgrad(A(dl), H, p.down, M, A(sc.du), I, o, dlq, GradQ{sc.duq, f8b_lin(p.up) ? a.g_du : -1});
    lin_wgrad(A(sc.du), I, A(x.x), H, p.up, M, true, WgQ8{duq, x});
    Opt o2; o2.addend = A(sc.dres_a); o2.ld_add = H;
    lin_dgrad(A(sc.du), I, p.up, M, A(gx), H, o2, duq);
    // wgrad_flush & 1: the FFN block's two weight gradients (and the LayerNorm column pass) leave for the side stream HERE, behind
    // the FFN-up data gradient, instead of at the end of the layer with the projection's and the QKV's: the grouped launch then runs
    // beside this layer's LayerNorm backward / attention-output dgrad / attention backward / QKV dgrad -- kernels of <= 156
    // workgroups -- and not beside the next layer's FFN data gradients.  Same kernels per problem, same sums: bit-identical.
    if (e->wgrad_flush & 1) flush_wgrads();
  }

  // ---------------------------------------------------------------- self-attention layer
  // layer `idx` of this Run's stack: the text layers run on the text stream's Run, the visual layers on the visual one (`which` is the
  // attention's kind)
  void self_fwd(int idx, const Act& x) {
    const SelfLayerP& p = (which ? e->vl : e->tl)[idx]; const SelfLayerA& a = (which ? e->vla : e->tla)[idx];
    const AttnSite at = site(which, idx, 0);
    const int M = b->B * at.Tq, H = p.H;
    lin_fwd(x, p.qkv.in, p.qkv, M, Act{a.qkv}, 3 * H, Opt());
    const Act ctx = ctx_act(at, p.proj.dense, attn_q_ok(at));
    attn_fwd(at, ctx);
    proj_fwd(p.proj, a.proj, ctx, x, M, drop(p.p_hid, p.site + 1));
    ffn_fwd(p.ffn, a.ffn, a.proj.out(p.proj.ln), M, drop(p.p_hid, p.site + 2));
  }
  // x: the layer input (its e4m3 copy serves the fp8 weight gradient of the QKV projection); g: grad of the output, gx: of x
  // dx = false (the lowest running step of its stream, SegPlan): gx has no reader and the launch that only produces it is not issued
  void self_bwd(int idx, const Act& x, size_t g, size_t gx, bool dx = true) {
    const SelfLayerP& p = (which ? e->vl : e->tl)[idx]; const SelfLayerA& a = (which ? e->vla : e->tla)[idx];
    const AttnSite at = site(which, idx, 0);
    const int M = b->B * at.Tq, H = p.H;
    const StreamScratch& sc = layer_begin();
    ffn_bwd(p.ffn, a.ffn, a.proj.out(p.proj.ln), g, sc.gc, sc, M, drop(p.p_hid, p.site + 2));
    const bool aq = attn_q_ok(at);
    const bool gq = aq && f8b_lin(p.qkv) && f8_lin(p.qkv);      // e5m2 copy of dqkv: fp8 data and weight gradient of the QKV projection
    const GradQ dqkvq{sc.dqkvq, gq ? a.g_dqkv : -1};
    proj_bwd(p.proj, a.proj, ctx_act(at, p.proj.dense, aq), sc.gc, sc, M, drop(p.p_hid, p.site + 1));
    attn_bwd(at, sc.dctx, sc.dqkv, sc.dqkv, dqkvq, dqkvq);
    attn_map_grads(at, sc.dqkv, sc.dqkv);
    lin_wgrad(A(sc.dqkv), 3 * H, A(x.x), H, p.qkv, M, true, WgQ8{dqkvq, x});
    Opt o; o.addend = A(sc.dres_b); o.ld_add = H;
    if (dx) lin_dgrad(A(sc.dqkv), 3 * H, p.qkv, M, A(gx), H, o, dqkvq);
    layer_end();
  }

  // ---------------------------------------------------------------- connection layer (vilbert.py:774-788)
  // `this` drives the TEXT stream, `V` the VISUAL stream (they may share one HIP stream).
  void conn_fwd(Run& V, int idx, const StepIn& x) {
    const ConnLayerP& p = e->cl[idx]; const ConnLayerA& a = e->cla[idx];
    const CrctModelDims& D = e->d;
    const int B = b->B, Mv = B * b->V, Mt = B * b->T, Hb = D.Hb;
    V.lin_fwd(x.v, p.qkv1.in, p.qkv1, Mv, Act{a.qkv1}, 3 * Hb, Opt());      // query1/key1/value1  :662-664
    lin_fwd(x.t, p.qkv2.in, p.qkv2, Mt, Act{a.qkv2}, 3 * Hb, Opt());        // query2/key2/value2  :673-675
    cross_sync(V);                                    // text needs k1, v1; visual needs k2, v2
    // text queries over visual keys/values -> ctx1 [B,T,Hb]  :684-701; visual queries over text keys/values -> ctx2 [B,V,Hb]  :704-723
    const AttnSite at = site(2, idx, 0), av = V.site(2, idx, 1);
    const bool aq = attn_q_ok(at) && attn_q_ok(av);
    const Act ctx1 = ctx_act(at, p.proj_t.dense, aq), ctx2 = V.ctx_act(av, p.proj_v.dense, aq);
    attn_fwd(at, ctx1);
    V.attn_fwd(av, ctx2);
    // cross wiring :780 -- visual stream takes ctx2, text stream takes ctx1
    V.proj_fwd(p.proj_v, a.proj_v, ctx2, x.v, Mv, drop(D.p_v_hidden, p.site + 2));
    proj_fwd(p.proj_t, a.proj_t, ctx1, x.t, Mt, drop(D.p_hidden, p.site + 3));
    V.ffn_fwd(p.ffn_v, a.ffn_v, a.proj_v.out(p.proj_v.ln), Mv, drop(D.p_v_hidden, p.site + 4));
    ffn_fwd(p.ffn_t, a.ffn_t, a.proj_t.out(p.proj_t.ln), Mt, drop(D.p_hidden, p.site + 5));
  }
  // x: the two layer inputs (their e4m3 copies serve the fp8 weight gradients of the QKV projections); gv / gt: grads of the two
  // outputs, gxv / gxt: of the inputs (dxv / dxt = false: not produced, as in self_bwd)
  void conn_bwd(Run& V, int idx, const StepIn& x, size_t gv, size_t gt, size_t gxv, size_t gxt, bool dxv = true, bool dxt = true) {
    const ConnLayerP& p = e->cl[idx]; const ConnLayerA& a = e->cla[idx];
    const CrctModelDims& D = e->d;
    hipEvent_t free_v = V.set_free[V.parity], free_t = set_free[parity];      // "the last readers of this scratch set are done"
    const StreamScratch& sv = V.layer_begin(); const StreamScratch& st = layer_begin();
    const int B = b->B, Mv = B * b->V, Mt = B * b->T, Hb = D.Hb;
    const AttnSite at = site(2, idx, 0), av = V.site(2, idx, 1);      // ctx1 = attn(q2, k1, v1) on the text stream, ctx2 = attn(q1, k2, v2) on the visual one
    V.ffn_bwd(p.ffn_v, a.ffn_v, a.proj_v.out(p.proj_v.ln), gv, sv.gc, sv, Mv, drop(D.p_v_hidden, p.site + 4));
    ffn_bwd(p.ffn_t, a.ffn_t, a.proj_t.out(p.proj_t.ln), gt, st.gc, st, Mt, drop(D.p_hidden, p.site + 5));
    const bool aq = attn_q_ok(at) && attn_q_ok(av);
    // e5m2 copies of the two fused dqkv buffers: only when BOTH QKV projections run their gradients in fp8 (each buffer is written by
    // both attention kernels)
    const bool gq = aq && f8b_lin(p.qkv1) && f8b_lin(p.qkv2) && f8_lin(p.qkv1) && f8_lin(p.qkv2);
    const GradQ dqkvq_v{sv.dqkvq, gq ? a.g_dqkv1 : -1}, dqkvq_t{st.dqkvq, gq ? a.g_dqkv2 : -1};
    V.proj_bwd(p.proj_v, a.proj_v, V.ctx_act(av, p.proj_v.dense, aq), sv.gc, sv, Mv, drop(D.p_v_hidden, p.site + 2));   // dctx2 [Mv,Hb]
    proj_bwd(p.proj_t, a.proj_t, ctx_act(at, p.proj_t.dense, aq), st.gc, st, Mt, drop(D.p_hidden, p.site + 3));         // dctx1 [Mt,Hb]
    // each attention backward also writes into the OTHER stream's dqkv scratch, which the layer that used this scratch set
    // last (its dgrad, and its weight-gradient GEMMs on the side stream) may still be reading.  With side streams that
    // layer's end is marked by the set's free event (recorded on the side stream behind everything the layer enqueued):
    // each data stream also waits for the OTHER side's event -- long signalled, so the wait is free, where a fresh
    // two-way hand-off costs 10+ us on the critical stream (tools/handoff_lab.cpp).  Without side streams: a full ordering.
    if (sw != s && V.sw != V.s) {
      if (free_v && !rc && hipStreamWaitEvent(s, free_v, 0) != hipSuccess) { crct_set_error("engine: stream wait failed"); rc = 1; }
      if (free_t && !V.rc && hipStreamWaitEvent(V.s, free_t, 0) != hipSuccess) { crct_set_error("engine: stream wait failed"); V.rc = 1; }
    } else cross_sync(V);
    // ctx1 = attn(q2, k1, v1): dq2 -> dqkv2[:, 0:Hb], dk1/dv1 -> dqkv1[:, Hb:3Hb]            (text stream)
    attn_bwd(at, st.dctx, st.dqkv, sv.dqkv, dqkvq_t, dqkvq_v);
    // ctx2 = attn(q1, k2, v2): dq1 -> dqkv1[:, 0:Hb], dk2/dv2 -> dqkv2[:, Hb:3Hb]            (visual stream)
    V.attn_bwd(av, sv.dctx, sv.dqkv, st.dqkv, dqkvq_v, dqkvq_t);
    // the requested maps of the two attentions, each behind its own backward on that stream and onto the very columns it wrote
    attn_map_grads(at, st.dqkv, sv.dqkv);
    V.attn_map_grads(av, sv.dqkv, st.dqkv);
    // each stream's dqkv buffer has been written by BOTH attention backward kernels
    cross_sync(V);
    V.lin_wgrad(A(sv.dqkv), 3 * Hb, A(x.v.x), D.Hv, p.qkv1, Mv, true, WgQ8{dqkvq_v, x.v});
    Opt ov; ov.addend = A(sv.dres_b); ov.ld_add = D.Hv;
    if (dxv) V.lin_dgrad(A(sv.dqkv), 3 * Hb, p.qkv1, Mv, A(gxv), D.Hv, ov, dqkvq_v);
    lin_wgrad(A(st.dqkv), 3 * Hb, A(x.t.x), D.H, p.qkv2, Mt, true, WgQ8{dqkvq_t, x.t});
    Opt ot; ot.addend = A(st.dres_b); ot.ld_add = D.H;
    if (dxt) lin_dgrad(A(st.dqkv), 3 * Hb, p.qkv2, Mt, A(gxt), D.H, ot, dqkvq_t);
    V.layer_end();
    layer_end();
  }

  // ---------------------------------------------------------------- embeddings
  void embed_text_fwd() {
    const CrctModelDims& D = e->d;
    const Drop dt = drop(D.p_hidden, 1);       // hidden_dropout_prob (vilbert.py:315)
    if (!rc) fail(crct_embed_text_fwd(b->tokens, b->segments, b->loc, P(e->et.word), P(e->et.pos), P(e->et.type), P(e->et.wloc),
                                      P(e->et.bloc), P(e->et.ln.g), P(e->et.ln.b), A(e->eta.sum), A(e->eta.y), F(e->eta.mean),
                                      F(e->eta.rstd), b->B, b->T, D.H, D.n_pos, 1e-12f, dt.thr, dt.scale, dt.site, c->seed, s));
    if (!rc && f8()) fail(crct_fp8_quantize_bf16(A(e->eta.y), W<uint8_t>(e->eta.yq), ascale(e->eta.site), aamax(e->eta.site),
                                                 (int64_t)b->B * b->T * D.H, s));
  }
  void embed_image_fwd() {
    const CrctModelDims& D = e->d;
    const int Mv = b->B * b->V;
    const Drop dv = drop(D.p_hidden, 2);       // also the TEXT probability (vilbert.py:1470)
    if (!e->feat) {                            // 'dvqa' / 'figure_qa': no feature term, the features are not read (vilbert.py:1481-1483)
      const bool ar = e->areas != nullptr;
      if (!rc) fail(crct_embed_image_var_fwd(b->image_loc, b->image_target, e->areas, P(e->ev.wloc), P(e->ev.bloc), P(e->ev.color),
                                             ar ? P(e->ev.areas.w) : nullptr, ar ? P(e->ev.areas.b) : nullptr, P(e->ev.ln.g), P(e->ev.ln.b),
                                             A(e->eva.sum), A(e->eva.y), F(e->eva.mean), F(e->eva.rstd), Mv, D.Hv, 1e-12f, dv.thr, dv.scale,
                                             dv.site, c->seed, s));
      return;
    }
    if (!rc) fail(b->image_feat_bf16 ? crct_softmax_rows_bf16_bf16(b->image_feat, A(e->eva.soft), Mv, D.Fv, s)
                                     : crct_softmax_rows_f32_bf16((const float*)b->image_feat, A(e->eva.soft), Mv, D.Fv, s));
    lin_fwd(Act{e->eva.soft}, D.Fv, e->ev.img, Mv, Act{e->eva.lin}, D.Hv, Opt());
    if (!rc) fail(crct_embed_image_fwd(A(e->eva.lin), b->image_loc, b->image_target, P(e->ev.wloc), P(e->ev.bloc), P(e->ev.color),
                                       P(e->ev.ln.g), P(e->ev.ln.b), A(e->eva.sum), A(e->eva.y), F(e->eva.mean), F(e->eva.rstd),
                                       Mv, D.Hv, 1e-12f, dv.thr, dv.scale, dv.site, c->seed, s));
    if (!rc && f8()) fail(crct_fp8_quantize_bf16(A(e->eva.y), W<uint8_t>(e->eva.yq), ascale(e->eva.site), aamax(e->eva.site),
                                                 (int64_t)Mv * D.Hv, s));
  }
  void embed_text_bwd(size_t gt) {
    const CrctModelDims& D = e->d;
    const Drop dt = drop(D.p_hidden, 1);
    layer_begin();
    ++tick;
    if (!rc) fail(crct_embed_text_bwd_indexed(A(gt), A(e->eta.sum), F(e->eta.mean), F(e->eta.rstd), b->tokens, b->segments, b->loc,
                                              P(e->et.ln.g), e->grad_at(e->et.word) ? G(e->et.word) : nullptr, G(e->et.pos), G(e->et.type), G(e->et.wloc), G(e->et.bloc),
                                              G(e->et.ln.g), G(e->et.ln.b), F(partials), b->B, b->T, D.H, D.n_pos, dt.thr, dt.scale,
                                              dt.site, c->seed, F(e->embed_rows[0]), W<int32_t>(e->embed_idx[0]), D.n_types, e->word_index,
                                              D.vocab, s));
  }
  void embed_image_bwd(size_t gv) {
    const CrctModelDims& D = e->d;
    const int Mv = b->B * b->V;
    const Drop dv = drop(D.p_hidden, 2);
    const StreamScratch& sc = layer_begin();
    ++tick;
    if (!e->feat) {
      const bool ar = e->areas != nullptr;
      if (!rc) fail(crct_embed_image_var_bwd(A(gv), A(e->eva.sum), F(e->eva.mean), F(e->eva.rstd), b->image_loc, b->image_target, e->areas,
                                             P(e->ev.ln.g), G(e->ev.color), G(e->ev.wloc), G(e->ev.bloc), ar ? G(e->ev.areas.w) : nullptr,
                                             ar ? G(e->ev.areas.b) : nullptr, G(e->ev.ln.g), G(e->ev.ln.b), F(partials), Mv, D.Hv, dv.thr,
                                             dv.scale, dv.site, c->seed, F(e->embed_rows[1]), W<int32_t>(e->embed_idx[1]), D.n_color, s));
      return;
    }
    if (!rc) fail(crct_embed_image_bwd(A(gv), A(e->eva.sum), F(e->eva.mean), F(e->eva.rstd), b->image_loc, b->image_target,
                                       P(e->ev.ln.g), A(sc.gc), G(e->ev.color), G(e->ev.wloc), G(e->ev.bloc), G(e->ev.img.b),
                                       G(e->ev.ln.g), G(e->ev.ln.b), F(partials), Mv, D.Hv, dv.thr, dv.scale, dv.site,
                                       c->seed, F(e->embed_rows[1]), W<int32_t>(e->embed_idx[1]), D.n_color, s));
    lin_wgrad(A(sc.gc), D.Hv, A(e->eva.soft), D.Fv, e->ev.img, Mv);   // the features are inputs: their gradient only on request (embed_image_input_grads)
  }
  // The gradients of the embeddings' float inputs (crct_engine_set_input_grads), after the half's own backward on its stream.
  void embed_text_input_grads(size_t gt) {
    const CrctModelDims& D = e->d;
    const Drop dt = drop(D.p_hidden, 1);
    ++tick;
    if (!rc) fail(crct_embed_input_grad(A(gt), A(e->eta.sum), F(e->eta.mean), F(e->eta.rstd), P(e->et.ln.g), b->loc, P(e->et.wloc), nullptr,
                                        e->req.ig.d_txt_loc, nullptr, e->req.ig.d_text_emb, b->B * b->T, D.H, dt.thr, dt.scale, dt.site, c->seed, s));
  }
  // ... image rows: d_loc and d_areas from the row kernel; the features' gradient through new_image_embeddings and the softmax:
  // g[Mv][Fv] = d_sum W as fp32 (its bf16 rounding would sit in front of the softmax backward's cancelling difference) from the bf16
  // d_sum in this layer's gc that the weight-gradient GEMM reads too -- always the bf16 kernel: this Linear has no e4m3 shadow
  void embed_image_input_grads(size_t gv) {
    const CrctModelDims& D = e->d;
    const int Mv = b->B * b->V;
    const Drop dv = drop(D.p_hidden, 2);
    if (e->req.ig.d_image_loc || e->req.ig.d_areas) {
      ++tick;
      if (!rc) fail(crct_embed_input_grad(A(gv), A(e->eva.sum), F(e->eva.mean), F(e->eva.rstd), P(e->ev.ln.g), nullptr, P(e->ev.wloc),
                                          e->req.ig.d_areas ? P(e->ev.areas.w) : nullptr, e->req.ig.d_image_loc, e->req.ig.d_areas, nullptr, Mv, D.Hv,
                                          dv.thr, dv.scale, dv.site, c->seed, s));
    }
    if (!e->req.ig.d_image_feat) return;
    const StreamScratch& sc = *sets[parity];               // the set embed_image_bwd has just written (layer_begin does not advance it)
    float* g = F(e->ws_base());
    Opt o; o.f32 = true;
    lin_dgrad(A(sc.gc), D.Hv, e->ev.img, Mv, g, D.Fv, o);
    ++tick;
    if (!rc) fail(crct_softmax_bwd_rows(b->image_feat, b->image_feat_bf16, g, e->req.ig.d_image_feat, Mv, D.Fv, s));
  }

  // ---------------------------------------------------------------- heads
  void pipe_fwd(const LinearP* l, size_t x0, int64_t ldx0, const size_t* acts, size_t out_last, int64_t ld_last, int B) {
    // Linear+LeakyReLU x3, then a plain Linear into `out_last` (regressor.py:8-28)
    Opt o; o.act = ACT_LEAKY;
    lin_fwd(Act{x0}, ldx0, l[0], B, Act{acts[0]}, l[0].out, o);
    lin_fwd(Act{acts[0]}, l[0].out, l[1], B, Act{acts[1]}, l[1].out, o);
    lin_fwd(Act{acts[1]}, l[1].out, l[2], B, Act{acts[2]}, l[2].out, o);
    lin_fwd(Act{acts[2]}, l[2].out, l[3], B, Act{out_last}, ld_last, Opt());
  }
  // backward of a pipe: du3 = grad of the last Linear's output (ld = ld3); writes dx0 (+= if acc).  gb = three gradient
  // buffers of this pipe alone (nothing is recycled: the weight-gradient GEMMs that read them run later, on the side stream)
  void pipe_bwd(const LinearP* l, const bf16_t* x0, int64_t ldx0, const size_t* acts, const bf16_t* du3, int64_t ld3,
                bf16_t* dx0, int64_t lddx0, bool acc0, int B, const size_t* gb) {
    bias_grad(du3, ld3, l[3], B);
    lin_wgrad(du3, ld3, A(acts[2]), l[2].out, l[3], B);
    Opt o; o.dact = ACT_LEAKY; o.dact_src = A(acts[2]); o.ld_aux = l[2].out;
    lin_dgrad(du3, ld3, l[3], B, A(gb[0]), l[2].out, o);                      // du2
    bias_grad(A(gb[0]), l[2].out, l[2], B);
    lin_wgrad(A(gb[0]), l[2].out, A(acts[1]), l[1].out, l[2], B);
    o.dact_src = A(acts[1]); o.ld_aux = l[1].out;
    lin_dgrad(A(gb[0]), l[2].out, l[2], B, A(gb[1]), l[1].out, o);            // du1
    bias_grad(A(gb[1]), l[1].out, l[1], B);
    lin_wgrad(A(gb[1]), l[1].out, A(acts[0]), l[0].out, l[1], B);
    o.dact_src = A(acts[0]); o.ld_aux = l[0].out;
    lin_dgrad(A(gb[1]), l[1].out, l[1], B, A(gb[2]), l[0].out, o);            // du0
    bias_grad(A(gb[2]), l[0].out, l[0], B);
    lin_wgrad(A(gb[2]), l[0].out, x0, ldx0, l[0], B);
    if (dx0) { Opt od; od.acc = acc0; lin_dgrad(A(gb[2]), l[0].out, l[0], B, dx0, lddx0, od); }
  }

  // Heads, forward.  The pooler and the regressor pipe of a stream only need that stream's last hidden states, so each data
  // stream runs its own branch (this = text or visual Run) before the two join for the fusion MLP and the loss kernel.
  void heads_branch_fwd(bool visual, size_t seq) {
    const CrctModelDims& D = e->d;
    const int B = b->B;
    const int64_t ld = visual ? (int64_t)b->V * D.Hv : (int64_t)b->T * D.H;  // CLS / IMG rows: hidden_states[:, 0]
    Opt orelu; orelu.act = ACT_RELU;
    if (visual) {
      lin_fwd(Act{seq}, ld, e->v_pool, B, Act{e->ha.pooled_v}, D.Hb, orelu);   // vilbert.py:970-976
      if (has_regressor())
        pipe_fwd(e->vp, seq, ld, e->ha.v, e->ha.cat, 512, B);                // regressor on the raw IMG state; cat = (hv, hw): regressor.py:39-41
    } else {
      lin_fwd(Act{seq}, ld, e->t_pool, B, Act{e->ha.pooled_t}, D.Hb, orelu);   // vilbert.py:955-961
      if (has_regressor()) pipe_fwd(e->tp, seq, ld, e->ha.t, e->ha.cat + 256 * sizeof(bf16_t), 512, B);
    }
  }
  bool has_regressor() const { return e->var.regressor != CRCT_REGRESSOR_NONE; }
  bool plain_head() const { return e->var.dataset == CRCT_DATASET_PLOTQA && e->var.regressor == CRCT_REGRESSOR_PLOTQA; }
  // the loss kernel: crct_head_loss for the PlotQA model, crct_head_loss_variant otherwise; `scores`: the standing request of
  // crct_engine_set_score_grads (backward only), NULL = the plain launch
  int head_loss(const CrctHeadArgs& h, const CrctScoreGrads* scores = nullptr) {
    if (plain_head()) return crct_head_loss_scores(&h, scores, s);
    CrctHeadVariantArgs va;
    memset(&va, 0, sizeof(va));
    va.h = h; va.variant = e->var;
    va.snap = e->var.dataset == CRCT_DATASET_DVQA && e->var.regressor == CRCT_REGRESSOR_PLOTQA && !c->training;   // vilbert.py:1619-1625
    va.ce_scratch = e->var.regressor == CRCT_REGRESSOR_CE ? F(e->ha.ce) : nullptr;
    return crct_head_loss_variant_scores(&va, scores, s);
  }
  void fill_head_args(CrctHeadArgs& h, float* logits, float* reg, float* stats, bool with_grad) {
    const CrctModelDims& D = e->d;
    memset(&h, 0, sizeof(h));
    h.pooled_t = A(e->ha.pooled_t); h.pooled_v = A(e->ha.pooled_v); h.fus_h = A(e->ha.f[2]);
    h.w_cls = P(e->cls.w); h.b_cls = P(e->cls.b);
    if (has_regressor()) { h.w_f6 = P(e->fu[3].w); h.b_f6 = P(e->fu[3].b); }
    h.R = b->R; h.labels = b->labels; h.logits = logits; h.reg = reg; h.stats = stats; h.scratch = F(e->ha.scratch);
    if (with_grad && g32) {
      h.d_pooled_t = A(e->ha.d_pt); h.d_pooled_v = A(e->ha.d_pv); h.d_fus_h = A(e->ha.g[0]);
      h.d_w_cls = G(e->cls.w); h.d_b_cls = G(e->cls.b);
      if (has_regressor()) { h.d_w_f6 = G(e->fu[3].w); h.d_b_f6 = G(e->fu[3].b); }
    }
    h.g_nsp_dev = c->g_nsp_dev; h.g_reg_dev = c->g_reg_dev; h.g_loss_dev = c->g_loss_dev;
    h.B = b->B; h.Hb = D.Hb; h.fusion_sum = D.fusion_sum; h.use_l1 = c->use_l1; h.kind_l1 = c->kind_l1;
    h.tol_margin = c->tol_margin; h.nsp_coeff = c->nsp_coeff; h.reg_coeff = c->reg_coeff; h.grad_scale = c->grad_scale;
    const Drop dc = drop(D.p_cls, 3);
    h.drop_thr = dc.thr; h.drop_scale = dc.scale; h.drop_site = dc.site; h.seed = c->seed;
  }
  void heads_tail_fwd(float* logits, float* reg, float* stats) {
    const int B = b->B;
    Opt o; o.act = ACT_LEAKY;
    if (has_regressor()) {
      lin_fwd(Act{e->ha.cat}, 512, e->fu[0], B, Act{e->ha.f[0]}, 512, o);
      lin_fwd(Act{e->ha.f[0]}, 512, e->fu[1], B, Act{e->ha.f[1]}, 256, o);
      lin_fwd(Act{e->ha.f[1]}, 256, e->fu[2], B, Act{e->ha.f[2]}, 256, o);
    }
    if (rc) return;
    CrctHeadArgs h;
    fill_head_args(h, logits, reg, stats, false);
    fail(head_loss(h));
  }
  // Heads, backward (this = text stream, V = visual stream): fills the CLS / IMG rows of the running activation gradients
  // (other rows zero).  On the critical chain are only the loss kernel and the 13 small data-gradient GEMMs -- the visual
  // pooler / pipe on the visual stream beside the text ones; the 13 weight-gradient GEMMs and bias column sums are queued
  // for the side streams like those of every encoder layer (every gradient buffer below has ONE producer and is not
  // recycled within the call).
  void heads_bwd(Run& V, size_t seq_t, size_t seq_v, size_t gt, size_t gv, float* logits, float* reg, float* stats) {
    const CrctModelDims& D = e->d;
    const int B = b->B;
    const int64_t ldt = (int64_t)b->T * D.H, ldv = (int64_t)b->V * D.Hv;
    const size_t* g = e->ha.g;
    // the loss kernel is re-run with gradient outputs enabled (cheap: B rows) so that forward can be called alone for evaluation
    {
      CrctHeadArgs h;
      fill_head_args(h, logits, reg, stats, true);
      if (!rc) fail(head_loss(h, e->req.sg.d_logits || e->req.sg.d_value ? &e->req.sg : nullptr));
    }
    if (rc) return;
    if (!V.rc) V.fail(order_streams(e, s, V.s));                              // d_pooled_v is ready
    if (hipMemsetAsync(A(gt), 0, (size_t)B * b->T * D.H * 2, s) != hipSuccess ||
        hipMemsetAsync(V.A(gv), 0, (size_t)B * b->V * D.Hv * 2, V.s) != hipSuccess) { crct_set_error("engine: memset failed"); rc = 1; return; }
    ++tick; ++V.tick;
    // poolers (gradients already w.r.t. the pre-activations)
    bias_grad(A(e->ha.d_pt), D.Hb, e->t_pool, B);
    lin_wgrad(A(e->ha.d_pt), D.Hb, A(seq_t), ldt, e->t_pool, B);
    lin_dgrad(A(e->ha.d_pt), D.Hb, e->t_pool, B, A(gt), ldt, Opt());
    V.bias_grad(V.A(e->ha.d_pv), D.Hb, e->v_pool, B);
    V.lin_wgrad(V.A(e->ha.d_pv), D.Hb, V.A(seq_v), ldv, e->v_pool, B);
    V.lin_dgrad(V.A(e->ha.d_pv), D.Hb, e->v_pool, B, V.A(gv), ldv, Opt());
    if (!has_regressor()) {                    // binary answers: the poolers are the whole head
      output_grads(V, gt, gv);
      flush_wgrads();
      V.flush_wgrads();
      return;
    }
    // fusion MLP: g[0] = grad of fusion.4's pre-activation (from the loss kernel)
    bias_grad(A(g[0]), 256, e->fu[2], B);
    lin_wgrad(A(g[0]), 256, A(e->ha.f[1]), 256, e->fu[2], B);
    Opt o; o.dact = ACT_LEAKY; o.dact_src = A(e->ha.f[1]); o.ld_aux = 256;
    lin_dgrad(A(g[0]), 256, e->fu[2], B, A(g[1]), 256, o);                     // d fusion.2 pre-act
    bias_grad(A(g[1]), 256, e->fu[1], B);
    lin_wgrad(A(g[1]), 256, A(e->ha.f[0]), 512, e->fu[1], B);
    o.dact_src = A(e->ha.f[0]); o.ld_aux = 512;
    lin_dgrad(A(g[1]), 256, e->fu[1], B, A(g[2]), 512, o);                     // d fusion.0 pre-act [B,512]
    bias_grad(A(g[2]), 512, e->fu[0], B);
    lin_wgrad(A(g[2]), 512, A(e->ha.cat), 512, e->fu[0], B);
    lin_dgrad(A(g[2]), 512, e->fu[0], B, A(g[3]), 512, Opt());                 // d cat [B,512] = (d hv, d hw)
    if (!rc && !V.rc) V.fail(order_streams(e, s, V.s));                        // d cat is ready
    // pipes; their input gradients accumulate onto the pooler's rows
    V.pipe_bwd(e->vp, V.A(seq_v), ldv, e->ha.v, V.A(g[3]), 512, V.A(gv), ldv, true, B, g + 4);
    pipe_bwd(e->tp, A(seq_t), ldt, e->ha.t, A(g[3]) + 256, 512, A(gt), ldt, true, B, g + 7);
    output_grads(V, gt, gv);
    flush_wgrads();
    V.flush_wgrads();
  }
  // Requested upstream gradients of the final hidden states (crct_engine_set_output_grads) onto the hidden gradients the heads have just
  // finished -- each on the stream that owns the buffer, behind the last head data gradient into it, and only where segment 0's plan
  // produces that gradient.  Called at both exits of heads_bwd; without a request it launches nothing.
  void output_grads(Run& V, size_t gt, size_t gv) {
    const SegPlan& pl = e->plan[e->lm_seg];
    if (e->req.og.d_seq_t && pl.dx_t && !rc) {
      fail(crct_hidden_grad_add(A(gt), e->req.og.d_seq_t, c->grad_scale, (int64_t)b->B * b->T * e->d.H, s));
      ++tick;
    }
    if (e->req.og.d_seq_v && pl.dx_v && !V.rc) {
      V.fail(crct_hidden_grad_add(V.A(gv), e->req.og.d_seq_v, c->grad_scale, (int64_t)b->B * b->V * e->d.Hv, V.s));
      ++V.tick;
    }
  }
};

int check_batch(const crct_engine* e, const CrctBatch* b) {
  CRCT_REQUIRE(b && b->B >= 1 && b->T >= 1 && b->V >= 1, "engine: bad batch sizes");
  CRCT_REQUIRE(b->B <= e->maxB && b->T <= e->maxT && b->V <= e->maxV, "engine: batch (B=%d,T=%d,V=%d) exceeds the engine maximum (%d,%d,%d)",
               b->B, b->T, b->V, e->maxB, e->maxT, e->maxV);
  CRCT_REQUIRE(b->tokens && b->segments && b->loc && b->image_feat && b->image_loc && b->image_target && b->R, "engine: null batch pointer");
  CRCT_REQUIRE(b->text_keymask || (b->sep_indices && b->hist_len && b->sep_stride > 0), "engine: text_keymask, or sep_indices + hist_len, is required");
  CRCT_REQUIRE(b->image_keymask || b->image_mask, "engine: image_keymask or image_mask is required");
  return 0;
}

// The backward plan, derived from the schedule and the set of tensors without gradient -- the one place the rules live:
//  * a schedule step runs iff a tensor with gradient lies in it or below it in the forward graph on a stream it touches (a
//    co-attention step touches both; the embeddings are the bottom step of their stream);
//  * the gradient of a step's text / visual input is produced iff something with gradient lies below that input;
//  * the last segment holds both embeddings: each half follows its own stream, and runs also for a requested gradient of one of its
//    float inputs (crct_engine_set_input_grads) -- which therefore keeps every step above it on that stream running;
//  * `dropped`: the weight-gradient GEMMs a running segment leaves out (crct_engine::drops_wgrad).
void replan(crct_engine* e) {
  const size_t nseg = e->sched.size() + 2 + e->lm_seg;
  e->plan.assign(nseg, SegPlan());
  if (e->lm_seg) e->plan[0].dx_t = e->plan[0].dx_v = false;      // the masked-LM head's segment: no launch of the engine's
  e->emb_own_t = e->emb_own_v = true;
  if (e->nograd.empty()) return;
  auto lin = [&](const LinearP& l) { return e->w_grad(l) || e->b_grad(l); };
  auto ln = [&](const LnP& l) { return e->grad_at(l.g) || e->grad_at(l.b); };
  auto proj = [&](const ProjP& p) { return lin(p.dense) || ln(p.ln); };
  auto ffn = [&](const FfnP& p) { return lin(p.up) || lin(p.down) || ln(p.ln); };
  auto drops = [&](const LinearP& l, bool with_bias) { return e->drops_wgrad(l, with_bias) ? 1 : 0; };
  auto self_drops = [&](const SelfLayerP& l) { return drops(l.qkv, true) + drops(l.proj.dense, false) + drops(l.ffn.up, true) + drops(l.ffn.down, false); };
  bool below_t = e->grad_at(e->et.word) || e->grad_at(e->et.pos) || e->grad_at(e->et.type) || e->grad_at(e->et.wloc) ||
                 e->grad_at(e->et.bloc) || ln(e->et.ln);
  bool below_v = (e->feat ? lin(e->ev.img) : lin(e->ev.areas)) || e->grad_at(e->ev.color) || e->grad_at(e->ev.wloc) ||
                 e->grad_at(e->ev.bloc) || ln(e->ev.ln);
  e->emb_own_t = below_t; e->emb_own_v = below_v;
  // a requested input gradient counts as something with gradient below the embeddings of its stream (crct_engine_set_input_grads)
  below_t = below_t || e->req.ig_text();
  below_v = below_v || e->req.ig_vis();
  SegPlan& emb = e->plan[nseg - 1];
  emb.runs = below_t || below_v; emb.dx_t = below_t; emb.dx_v = below_v;
  emb.dropped = (e->feat && below_v) ? drops(e->ev.img, false) : 0;      // (also when the half runs for an input gradient alone)
  for (size_t i = 0; i < e->sched.size(); ++i) {
    const Step& st = e->sched[i];
    SegPlan& pl = e->plan[e->sched.size() - i + e->lm_seg];
    pl.dx_t = below_t; pl.dx_v = below_v;
    if (st.kind == 't' || st.kind == 'v') {
      const SelfLayerP& l = st.kind == 't' ? e->tl[st.idx] : e->vl[st.idx];
      bool& below = st.kind == 't' ? below_t : below_v;
      pl.runs = below || lin(l.qkv) || proj(l.proj) || ffn(l.ffn);
      pl.dropped = pl.runs ? self_drops(l) : 0;
      below = pl.runs;
    } else {
      const ConnLayerP& l = e->cl[st.idx];
      pl.runs = below_t || below_v || lin(l.qkv1) || lin(l.qkv2) || proj(l.proj_v) || proj(l.proj_t) || ffn(l.ffn_v) || ffn(l.ffn_t);
      pl.dropped = !pl.runs ? 0 : drops(l.qkv1, true) + drops(l.qkv2, true) + drops(l.proj_v.dense, false) + drops(l.proj_t.dense, false) +
                                    drops(l.ffn_v.up, true) + drops(l.ffn_v.down, false) + drops(l.ffn_t.up, true) + drops(l.ffn_t.down, false);
      below_t = below_v = pl.runs;
    }
    if (!pl.runs) pl.dx_t = pl.dx_v = false;
  }
  // heads: both input gradients are the running activation gradients the encoder's backward starts from
  SegPlan& hd = e->plan[e->lm_seg];
  const bool reg = e->var.regressor != CRCT_REGRESSOR_NONE;
  bool own = lin(e->t_pool) || lin(e->v_pool) || lin(e->cls);
  int dropped = drops(e->t_pool, false) + drops(e->v_pool, false);
  for (int j = 0; j < 4 && reg; ++j) {
    own = own || lin(e->tp[j]) || lin(e->vp[j]) || lin(e->fu[j]);
    dropped += drops(e->tp[j], false) + drops(e->vp[j], false) + (j < 3 ? drops(e->fu[j], false) : 0);      // fusion.6: the head kernel's
  }
  hd.runs = own || below_t || below_v;
  hd.dx_t = hd.runs && below_t; hd.dx_v = hd.runs && below_v;
  hd.dropped = hd.runs ? dropped : 0;
}

}  // namespace

// =================================================================================== C ABI
extern "C" crct_engine_t* crct_engine_create_variant(const CrctModelDims* dims, const char* names, const int64_t* offsets,
                                                     const int64_t* sizes, int n_params, int max_B, int max_T, int max_V,
                                                     const CrctVariant* variant) {
  if (!dims || !names || !offsets || !sizes) { crct_set_error("engine_create: null argument"); return nullptr; }
  if (variant && (variant->dataset < CRCT_DATASET_PLOTQA || variant->dataset > CRCT_DATASET_FIGUREQA ||
                  variant->regressor < CRCT_REGRESSOR_PLOTQA || variant->regressor > CRCT_REGRESSOR_CE ||
                  variant->n_values < 0 || variant->n_values > CRCT_CE_CLASSES)) {
    crct_set_error("engine_create: bad variant (dataset %d, regressor %d, %d values)", variant->dataset, variant->regressor, variant->n_values);
    return nullptr;
  }
  if (variant && variant->regressor == CRCT_REGRESSOR_CE && variant->n_values != CRCT_CE_CLASSES) {
    crct_set_error("engine_create: the CE regressor needs the %d class values", CRCT_CE_CLASSES);
    return nullptr;
  }
  crct_engine* e = new crct_engine();
  e->d = *dims; e->maxB = max_B; e->maxT = max_T; e->maxV = max_V;
  if (variant) e->var = *variant;
  e->feat = e->var.dataset == CRCT_DATASET_PLOTQA;
  const CrctModelDims& D = e->d;
  {
    const char* p = names;
    for (int i = 0; i < n_params; ++i) {
      const char* q = strchr(p, '\n');
      std::string k = q ? std::string(p, q - p) : std::string(p);
      e->off[k] = offsets[i]; e->size[k] = sizes[i];
      e->param_off.push_back(offsets[i]);
      if (!q) break;
      p = q + 1;
    }
  }
  auto fail = [&](const char* msg) -> crct_engine_t* { if (msg) crct_set_error("%s", msg); delete e; return nullptr; };
  if (D.H % D.heads || D.Hv % D.v_heads || D.Hb % D.b_heads) return fail("engine_create: hidden size not a multiple of heads");
  if (D.H % 8 || D.Hv % 8 || D.Hb % 8 || D.I % 8 || D.Iv % 8 || D.Fv % 8) return fail("engine_create: sizes must be multiples of 8");
  if (D.n_conn > 32) return fail("engine_create: more than 32 connection layers");
  // ---- schedule (vilbert.py:852-939)
  {
    int vs = 0, ts = 0;
    for (int c = 0; c < D.n_conn; ++c) {
      for (int i = vs; i < D.v_biatt[c]; ++i) e->sched.push_back({'v', i});
      for (int i = ts; i < D.t_biatt[c]; ++i) e->sched.push_back({'t', i});
      if (D.with_coattention) e->sched.push_back({'c', c});
      vs = D.v_biatt[c]; ts = D.t_biatt[c];
    }
    for (int i = vs; i < D.Lv; ++i) e->sched.push_back({'v', i});
    for (int i = ts; i < D.L; ++i) e->sched.push_back({'t', i});
    for (size_t i = 0; i < e->sched.size() && e->first_conn < 0; ++i)
      if (e->sched[i].kind == 'c') e->first_conn = (int)i;
  }
  // ---- parameters
  char buf[256];
  uint32_t site = 16;
  for (int i = 0; i < D.L; ++i, site += 4) {
    snprintf(buf, sizeof(buf), "bert.encoder.layer.%d.", i);
    e->tl.push_back(self_layer_p(e, buf, D.H, D.I, D.heads, D.p_attn, D.p_hidden, site, CRCT_SITE_T_QKV));
  }
  for (int i = 0; i < D.Lv; ++i, site += 4) {
    snprintf(buf, sizeof(buf), "bert.encoder.v_layer.%d.", i);
    e->vl.push_back(self_layer_p(e, buf, D.Hv, D.Iv, D.v_heads, D.p_v_attn, D.p_v_hidden, site, CRCT_SITE_V_QKV));
  }
  for (int i = 0; i < D.n_conn; ++i) {
    snprintf(buf, sizeof(buf), "bert.encoder.c_layer.%d.", i);
    std::string p(buf);
    ConnLayerP l;
    l.site = site; site += 8;
    l.qkv1 = fused3(e, p + "biattention.query1", p + "biattention.key1", p + "biattention.value1", D.Hv, D.Hb, CRCT_SITE_C_QKV_V);
    l.qkv2 = fused3(e, p + "biattention.query2", p + "biattention.key2", p + "biattention.value2", D.H, D.Hb, CRCT_SITE_C_QKV_T);
    l.proj_v.dense = linear_p(e, p + "biOutput.dense1", D.Hb, D.Hv, CRCT_SITE_C_OUT_V); l.proj_v.ln = ln_p(e, p + "biOutput.LayerNorm1");
    l.proj_t.dense = linear_p(e, p + "biOutput.dense2", D.Hb, D.H, CRCT_SITE_C_OUT_T); l.proj_t.ln = ln_p(e, p + "biOutput.LayerNorm2");
    l.ffn_v.up = linear_p(e, p + "v_intermediate.dense", D.Hv, D.Iv, CRCT_SITE_V_FFN_UP);
    l.ffn_v.down = linear_p(e, p + "v_output.dense", D.Iv, D.Hv, CRCT_SITE_V_FFN_DN); l.ffn_v.ln = ln_p(e, p + "v_output.LayerNorm");
    l.ffn_t.up = linear_p(e, p + "t_intermediate.dense", D.H, D.I, CRCT_SITE_T_FFN_UP);
    l.ffn_t.down = linear_p(e, p + "t_output.dense", D.I, D.H, CRCT_SITE_T_FFN_DN); l.ffn_t.ln = ln_p(e, p + "t_output.LayerNorm");
    e->cl.push_back(l);
  }
  e->et.word = e->P("bert.embeddings.word_embeddings.weight");
  e->et.pos = e->P("bert.embeddings.position_embeddings.weight");
  e->et.type = e->P("bert.embeddings.plotqa_type_embeddings.weight");
  e->et.wloc = e->P("bert.embeddings.txt_location_embeddings.weight");
  e->et.bloc = e->P("bert.embeddings.txt_location_embeddings.bias");
  e->et.ln = ln_p(e, "bert.embeddings.LayerNorm");
  if (e->feat) e->ev.img = linear_p(e, "bert.v_embeddings.new_image_embeddings", D.Fv, D.Hv, CRCT_SITE_IMG_EMB);
  else e->ev.areas = linear_p(e, "bert.v_embeddings.areas_emp", 1, D.Hv);
  e->ev.color = e->P("bert.v_embeddings.color_emb.weight");
  e->ev.wloc = e->P("bert.v_embeddings.new_loc_emb.weight");
  e->ev.bloc = e->P("bert.v_embeddings.new_loc_emb.bias");
  e->ev.ln = ln_p(e, "bert.v_embeddings.LayerNorm");
  e->t_pool = linear_p(e, "bert.t_pooler.dense", D.H, D.Hb);
  e->v_pool = linear_p(e, "bert.v_pooler.dense", D.Hv, D.Hb);
  e->cls = linear_p(e, "cls.bi_seq_relationship", D.Hb, 2);
  {
    // regressor.py:5-34 (PlotQA_Regressor_v20: fusion, 1 output) / :45-79 (DVQA_Regressor_v20_CE: ce_fusion, 65 outputs); none with
    // binary answers (vilbert.py:1518)
    const bool ce = e->var.regressor == CRCT_REGRESSOR_CE;
    const int tw[5] = {D.H, D.H, 512, 256, 256}, vw[5] = {D.Hv, D.Hv, 512, 256, 256}, fw[5] = {512, 512, 256, 256, ce ? CRCT_CE_CLASSES : 1};
    for (int j = 0; j < 4 && e->var.regressor != CRCT_REGRESSOR_NONE; ++j) {
      snprintf(buf, sizeof(buf), "regressor.txt_pipe.%d", 2 * j); e->tp[j] = linear_p(e, buf, tw[j], tw[j + 1]);
      snprintf(buf, sizeof(buf), "regressor.vis_pipe.%d", 2 * j); e->vp[j] = linear_p(e, buf, vw[j], vw[j + 1]);
      snprintf(buf, sizeof(buf), "regressor.%s.%d", ce ? "ce_fusion" : "fusion", 2 * j); e->fu[j] = linear_p(e, buf, fw[j], fw[j + 1]);
    }
  }
  if (e->bad) return fail(nullptr);
  {
    auto own = [&](const LinearP& l) { e->wgrad_owned[l.w] = (int64_t)l.in * l.out; };
    each_encoder_linear(e, own);
    if (e->feat) own(e->ev.img);                   // (areas_emp: produced by the embedding kernel, accumulate-only)
    own(e->t_pool); own(e->v_pool);
    if (e->var.regressor != CRCT_REGRESSOR_NONE) {
      for (int j = 0; j < 4; ++j) { own(e->tp[j]); own(e->vp[j]); }
      for (int j = 0; j < 3; ++j) own(e->fu[j]);   // fusion.6 (fu[3]) and bi_seq_relationship are produced by the head kernel: accumulate-only
    }
  }
  {
    // fp8: every Linear of the encoder whose two dimensions are whole numbers of 128-deep fp8 K tiles gets an e4m3 weight shadow
    // and a scale slot
    auto slot = [&](const LinearP& l) {
      if (l.in % 128 != 0 || l.out % 128 != 0) return;      // forward contracts over `in`, the data gradient over `out`: whole fp8 K tiles both ways
      e->wq_slot[l.w] = (int)e->wq_list.size();
      e->wq_list.push_back({l.w, (int64_t)l.in * l.out});
    };
    each_encoder_linear(e, slot);
  }

  // ---- workspace
  Arena ar;
  const size_t Mt = (size_t)max_B * max_T, Mv = (size_t)max_B * max_V, B = max_B;
  e->eta.sum = ar.take(Mt * D.H * 2); e->eta.y = ar.take(Mt * D.H * 2); e->eta.mean = ar.take(Mt * 4); e->eta.rstd = ar.take(Mt * 4);
  e->eva.soft = ar.take(e->feat ? Mv * D.Fv * 2 : 0); e->eva.lin = ar.take(e->feat ? Mv * D.Hv * 2 : 0); e->eva.sum = ar.take(Mv * D.Hv * 2);
  e->eva.y = ar.take(Mv * D.Hv * 2); e->eva.mean = ar.take(Mv * 4); e->eva.rstd = ar.take(Mv * 4);
  e->eta.yq = ar.take(Mt * D.H); e->eva.yq = ar.take(Mv * D.Hv);
  e->eta.site = e->n_sites++; e->eva.site = e->n_sites++;
  e->taps.push_back({"emb.t", e->eta.y, 't'});
  e->taps.push_back({"emb.v", e->eva.y, 'v'});
  for (int i = 0; i < D.L; ++i) e->tla.push_back(self_layer_a(ar, Mt, D.H, D.I, D.heads, e->n_sites, e->n_gsites));
  for (int i = 0; i < D.Lv; ++i) e->vla.push_back(self_layer_a(ar, Mv, D.Hv, D.Iv, D.v_heads, e->n_sites, e->n_gsites));
  e->cla.resize(D.n_conn);
  for (int i = 0; i < D.n_conn; ++i) {
    ConnLayerA& a = e->cla[i];
    a.qkv1 = ar.take(Mv * 3 * D.Hb * 2); a.qkv2 = ar.take(Mt * 3 * D.Hb * 2);
    a.ctx1 = ar.take(Mt * D.Hb * 2); a.ctx2 = ar.take(Mv * D.Hb * 2);
    a.ctx1q = ar.take(Mt * D.Hb); a.ctx2q = ar.take(Mv * D.Hb);
    a.lse1 = ar.take(Mt * D.b_heads * 4); a.lse2 = ar.take(Mv * D.b_heads * 4);
    a.site_ctx1 = e->n_sites++; a.site_ctx2 = e->n_sites++; a.g_dqkv1 = e->n_gsites++; a.g_dqkv2 = e->n_gsites++;
    a.proj_v = proj_a(ar, Mv, D.Hv, e->n_sites, e->n_gsites); a.proj_t = proj_a(ar, Mt, D.H, e->n_sites, e->n_gsites);
    a.ffn_v = ffn_a(ar, Mv, D.Hv, D.Iv, e->n_sites, e->n_gsites); a.ffn_t = ffn_a(ar, Mt, D.H, D.I, e->n_sites, e->n_gsites);
  }
  e->ha.pooled_t = ar.take(B * D.Hb * 2); e->ha.pooled_v = ar.take(B * D.Hb * 2);
  e->ha.t[0] = ar.take(B * D.H * 2); e->ha.t[1] = ar.take(B * 512 * 2); e->ha.t[2] = ar.take(B * 256 * 2);
  e->ha.v[0] = ar.take(B * D.Hv * 2); e->ha.v[1] = ar.take(B * 512 * 2); e->ha.v[2] = ar.take(B * 256 * 2);
  e->ha.cat = ar.take(B * 512 * 2);
  e->ha.f[0] = ar.take(B * 512 * 2); e->ha.f[1] = ar.take(B * 256 * 2); e->ha.f[2] = ar.take(B * 256 * 2);
  e->ha.scratch = ar.take(B * 8 * 4);
  e->ha.ce = ar.take(e->var.regressor == CRCT_REGRESSOR_CE ? B * CRCT_CE_CLASSES * 4 : 0);
  e->ha.d_pt = ar.take(B * D.Hb * 2); e->ha.d_pv = ar.take(B * D.Hb * 2);
  {
    size_t w = 512;
    if ((size_t)D.H > w) w = D.H;
    if ((size_t)D.Hv > w) w = D.Hv;
    for (int k = 0; k < 10; ++k) e->ha.g[k] = ar.take(B * w * 2);
  }
  e->st = scratch_a(ar, Mt, D.H, D.I, D.Hb);
  e->sv = scratch_a(ar, Mv, D.Hv, D.Iv, D.Hb);
  e->st2 = scratch_a(ar, Mt, D.H, D.I, D.Hb);
  e->sv2 = scratch_a(ar, Mv, D.Hv, D.Iv, D.Hb);
  {
    size_t wmax = D.H > D.Hv ? D.H : D.Hv;
    for (int k = 0; k < 2; ++k) {
      e->partials[k] = ar.take((size_t)10 * 4 * CRCT_LN_BWD_MAX_BLOCKS * wmax * 4);   // [<= 9][4 waves x blocks][H]
    }
    e->embed_rows[0] = ar.take(Mt * D.H * 4);  e->embed_idx[0] = ar.take(2 * Mt * 4);
    e->embed_rows[1] = ar.take(Mv * D.Hv * 4); e->embed_idx[1] = ar.take(Mv * 4);
    size_t nmax = 3 * (size_t)D.Hb;
    if ((size_t)D.I > nmax) nmax = D.I;
    if ((size_t)D.Iv > nmax) nmax = D.Iv;
    if (3 * (size_t)D.H > nmax) nmax = 3 * (size_t)D.H;
    if (3 * (size_t)D.Hv > nmax) nmax = 3 * (size_t)D.Hv;
    if (nmax < 1024) nmax = 1024;
    for (int k = 0; k < 4; ++k) e->colsum_part[k] = ar.take((size_t)64 * nmax * 4);
  }
  e->km_t = ar.take(Mt); e->km_v = ar.take(Mv);      // uint8 key masks built from sep_indices / hist_len / image_mask (CrctBatch)
  {
    // split-K slab space per data stream: the narrow outputs (N <= the widest hidden size) with up to 4 slices; wider outputs
    // have enough tiles and are never split.  Ticket words: zeroed at the start of every engine call.
    const int Hmax = std::max(std::max(D.H, D.Hv), D.Hb);
    e->sk_ws_elems[0] = (size_t)crct_gemm_splitk_ws_elems((int)Mt, Hmax, 4);
    e->sk_ws_elems[1] = (size_t)crct_gemm_splitk_ws_elems((int)Mv, Hmax, 4);
    e->sk_tickets = std::max(crct_gemm_splitk_tickets((int)Mt, Hmax), crct_gemm_splitk_tickets((int)Mv, Hmax));
    e->sk_tickets = (e->sk_tickets + 3) / 4 * 4;
    for (int k = 0; k < 2; ++k) e->sk_ws[k] = ar.take(e->sk_ws_elems[k] * 4);
    e->sk_cnt[0] = ar.take((size_t)2 * e->sk_tickets * 4);      // [text | visual] in one block: one memset per call
    e->sk_cnt[1] = e->sk_cnt[0] + (size_t)e->sk_tickets * 4;
  }
  // the fp32 LayerNorm outputs of the two-output route lie behind everything else: the default route neither writes nor allocates them
  e->ws_core = ar.top;
  for (SelfLayerA& a : e->tla) { a.proj.a32 = ar.take(Mt * D.H * 4); a.ffn.y32 = ar.take(Mt * D.H * 4); }
  for (SelfLayerA& a : e->vla) { a.proj.a32 = ar.take(Mv * D.Hv * 4); a.ffn.y32 = ar.take(Mv * D.Hv * 4); }
  for (ConnLayerA& a : e->cla) {
    a.proj_v.a32 = ar.take(Mv * D.Hv * 4); a.ffn_v.y32 = ar.take(Mv * D.Hv * 4);
    a.proj_t.a32 = ar.take(Mt * D.H * 4); a.ffn_t.y32 = ar.take(Mt * D.H * 4);
  }
  e->ws_two_output = ar.top;
  e->req.ws_ig = e->feat ? align_up(Mv * D.Fv * 4, 256) : 0;
  e->req.ws_amg = align_up((size_t)max_B * std::max(D.heads, std::max(D.v_heads, D.b_heads)) * std::max(max_T, max_V) * 3 * 4, 256);
  e->ws_update();

  // ---- the hidden states every schedule step starts from (the last entry: the encoder's outputs), and the taps on them
  {
    StepIn x = {Act{e->eta.y, e->eta.yq, e->eta.site}, Act{e->eva.y, e->eva.yq, e->eva.site}};
    for (const Step& st : e->sched) {
      e->in.push_back(x);
      if (st.kind == 't') x.t = e->tla[st.idx].ffn.out(e->tl[st.idx].ffn.ln);
      else if (st.kind == 'v') x.v = e->vla[st.idx].ffn.out(e->vl[st.idx].ffn.ln);
      else { x.v = e->cla[st.idx].ffn_v.out(e->cl[st.idx].ffn_v.ln); x.t = e->cla[st.idx].ffn_t.out(e->cl[st.idx].ffn_t.ln); }
      snprintf(buf, sizeof(buf), "%c%d.t", st.kind, st.idx); e->taps.push_back({buf, x.t.x, 't'});
      snprintf(buf, sizeof(buf), "%c%d.v", st.kind, st.idx); e->taps.push_back({buf, x.v.x, 'v'});
    }
    e->in.push_back(x);
    e->taps.push_back({"seq_t", x.t.x, 't'});
    e->taps.push_back({"seq_v", x.v.x, 'v'});
    // the fused [rows, 3 H] q | k | v buffers the attention kernels (and crct_engine_attention_probs) read: "t<i>.qkv", "v<i>.qkv", and per
    // connection layer "c<i>.qkv1" (visual rows) / "c<i>.qkv2" (text rows)
    for (int i = 0; i < D.L; ++i) { snprintf(buf, sizeof(buf), "t%d.qkv", i); e->taps.push_back({buf, e->tla[i].qkv, 't', 3 * D.H}); }
    for (int i = 0; i < D.Lv; ++i) { snprintf(buf, sizeof(buf), "v%d.qkv", i); e->taps.push_back({buf, e->vla[i].qkv, 'v', 3 * D.Hv}); }
    for (int i = 0; i < D.n_conn; ++i) {
      snprintf(buf, sizeof(buf), "c%d.qkv1", i); e->taps.push_back({buf, e->cla[i].qkv1, 'v', 3 * D.Hb});
      snprintf(buf, sizeof(buf), "c%d.qkv2", i); e->taps.push_back({buf, e->cla[i].qkv2, 't', 3 * D.Hb});
    }
  }

  // ---- gradient segments in backward order: heads, schedule reversed, embeddings
  auto range_of = [&](std::vector<std::string> prefixes) {
    int64_t lo = INT64_MAX, hi = -1;
    for (auto& kv : e->off)
      for (auto& pf : prefixes)
        if (kv.first.compare(0, pf.size(), pf) == 0 && e->size[kv.first] > 0) {    // size 0 = never receives a gradient
          if (kv.second < lo) lo = kv.second;
          const int64_t end = kv.second + e->size[kv.first];
          if (end > hi) hi = end;
        }
    if (hi < 0) { lo = 0; hi = 0; }
    return std::make_pair(lo, hi);
  };
  {
    // ONE launch-free segment for the masked-LM head and the masked-region head (cls.imagePredictions.*, params['img_loss_coeff'] > 0),
    // whichever is on: their tensors are adjacent in the tail of the buffers
    const auto lm = range_of({"cls.predictions.", "cls.imagePredictions."});
    if (lm.second > lm.first) { e->lm_seg = 1; e->seg_range.push_back(lm); }
  }
  e->seg_range.push_back(range_of({"bert.t_pooler.", "bert.v_pooler.", "cls.bi_seq_relationship.", "regressor."}));
  for (int i = (int)e->sched.size() - 1; i >= 0; --i) {
    const Step& st = e->sched[i];
    snprintf(buf, sizeof(buf), "bert.encoder.%s.%d.", st.kind == 't' ? "layer" : (st.kind == 'v' ? "v_layer" : "c_layer"), st.idx);
    e->seg_range.push_back(range_of({std::string(buf)}));
  }
  e->seg_range.push_back(range_of({"bert.embeddings.", "bert.v_embeddings."}));
  replan(e);
  return e;
}

extern "C" crct_engine_t* crct_engine_create(const CrctModelDims* dims, const char* names, const int64_t* offsets,
                                             const int64_t* sizes, int n_params, int max_B, int max_T, int max_V) {
  return crct_engine_create_variant(dims, names, offsets, sizes, n_params, max_B, max_T, max_V, nullptr);
}
extern "C" int crct_engine_set_areas(crct_engine_t* e, const float* areas) {
  CRCT_REQUIRE(e, "engine_set_areas: null engine");
  CRCT_REQUIRE(!areas || !e->feat, "engine_set_areas: the 'plotqa' image embeddings have no areas term (vilbert.py:1463-1465)");
  e->areas = areas;
  return 0;
}

extern "C" int crct_engine_set_input_grads(crct_engine_t* e, const CrctInputGrads* req) {
  CRCT_REQUIRE(e, "engine_set_input_grads: null engine");
  const CrctInputGrads r = req ? *req : Requests().ig;
  CRCT_REQUIRE(!r.d_image_feat || e->feat, "engine_set_input_grads: d_image_feat: the 'dvqa' / 'figure_qa' image embeddings never read the features (vilbert.py:1481-1483)");
  CRCT_REQUIRE(!r.d_areas || !e->feat, "engine_set_input_grads: d_areas: the 'plotqa' image embeddings have no areas term (vilbert.py:1463-1465)");
  const bool text = e->req.ig_text(), vis = e->req.ig_vis();
  e->req.ig = r;
  e->ws_update();
  if (text != e->req.ig_text() || vis != e->req.ig_vis()) replan(e);      // a requested input gradient keeps its stream's segments running
  return 0;
}

extern "C" int crct_engine_set_score_grads(crct_engine_t* e, const CrctScoreGrads* req) {
  CRCT_REQUIRE(e, "engine_set_score_grads: null engine");
  const CrctScoreGrads r = req ? *req : Requests().sg;
  CRCT_REQUIRE(!r.d_value || e->var.regressor == CRCT_REGRESSOR_PLOTQA, "engine_set_score_grads: d_value: only the PlotQA regressor's value has a gradient (this engine's regressor is %s)",
               e->var.regressor == CRCT_REGRESSOR_CE ? "the CE table lookup" : "absent");
  e->req.sg = r;
  return 0;
}

extern "C" int crct_engine_set_attention_map_grads(crct_engine_t* e, const CrctAttnMapGrad* req, int n) {
  CRCT_REQUIRE(e, "engine_set_attention_map_grads: null engine");
  CRCT_REQUIRE(n >= 0 && (req || n == 0), "engine_set_attention_map_grads: %d requests without an array", n);
  for (int i = 0; req && i < n; ++i) {
    AttnSite at;
    if (int r = e->attn_site("engine_set_attention_map_grads", req[i].kind, req[i].index, req[i].direction, 1, 1, &at)) return r;
    CRCT_REQUIRE(req[i].d_probs && (uintptr_t)req[i].d_probs % 4 == 0, "engine_set_attention_map_grads: request %d: d_probs must be a 4-byte aligned device buffer", i);
  }
  e->req.amg.assign(req, req + (req ? n : 0));
  e->ws_update();
  return 0;
}

extern "C" int crct_engine_set_output_grads(crct_engine_t* e, const CrctOutputGrads* req) {
  CRCT_REQUIRE(e, "engine_set_output_grads: null engine");
  const CrctOutputGrads r = req ? *req : Requests().og;
  CRCT_REQUIRE((((uintptr_t)r.d_seq_t | (uintptr_t)r.d_seq_v) & 15) == 0, "engine_set_output_grads: d_seq_t / d_seq_v must be 16-byte aligned");
  e->req.og = r;
  return 0;
}

extern "C" int crct_engine_sequence_outputs(crct_engine_t* e, const float* params_f32, const void* workspace, int B, int T, int V,
                                            float* seq_t, float* seq_v, crct_stream_t stream) {
  CRCT_REQUIRE(e && params_f32 && workspace, "engine_sequence_outputs: null argument");
  CRCT_REQUIRE(e->fwd_r32 >= 0, "engine_sequence_outputs: no crct_engine_forward has run on this engine");
  CRCT_REQUIRE(B >= 1 && T >= 1 && V >= 1 && B <= e->maxB && T <= e->maxT && V <= e->maxV,
               "engine_sequence_outputs: batch (B=%d,T=%d,V=%d) outside the engine maximum (%d,%d,%d)", B, T, V, e->maxB, e->maxT, e->maxV);
  const char* ws = (const char*)workspace;
  // the closing LayerNorm of a stream's last schedule step: the rows it normalised, their statistics, its parameters
  auto rebuild = [&](const Act& x, float* out, int64_t M, int H) -> int {
    if (!out) return 0;
    CRCT_REQUIRE(x.s != NONE, "engine_sequence_outputs: the stream has no encoder layer (its final state is the embeddings' bf16 output)");
    return crct_layernorm_rows_f32(ws + x.s, e->fwd_r32 ? 0 : 1, (const float*)(ws + x.mean), (const float*)(ws + x.rstd),
                                   params_f32 + x.ln.g, params_f32 + x.ln.b, out, (int)M, H, stream);
  };
  if (int r = rebuild(e->in.back().t, seq_t, (int64_t)B * T, e->d.H)) return r;
  return rebuild(e->in.back().v, seq_v, (int64_t)B * V, e->d.Hv);
}

extern "C" int crct_engine_set_trainable(crct_engine_t* e, const uint8_t* flags, int n) {
  CRCT_REQUIRE(e, "engine_set_trainable: null engine");
  CRCT_REQUIRE(!flags || n == (int)e->param_off.size(), "engine_set_trainable: %d flags for %d parameters", n, (int)e->param_off.size());
  e->nograd.clear();
  for (int i = 0; flags && i < n; ++i)
    if (!flags[i]) e->nograd.insert(e->param_off[i]);
  replan(e);
  return 0;
}
extern "C" int crct_engine_backward_plan(const crct_engine_t* e, int32_t* plan, int cap_segments) {
  if (!e) return -1;
  const int n = (int)e->plan.size();
  for (int i = 0; plan && i < n && i < cap_segments; ++i) {
    const SegPlan& p = e->plan[i];
    plan[4 * i] = p.runs; plan[4 * i + 1] = p.dx_t; plan[4 * i + 2] = p.dx_v; plan[4 * i + 3] = p.dropped;
  }
  return n;
}

extern "C" void crct_engine_destroy(crct_engine_t* e) {
  if (!e) return;
  for (auto ev : e->evpool) (void)hipEventDestroy(ev);
  for (auto st : e->side) if (st) (void)hipStreamDestroy(st);
  if (e->aux) (void)hipStreamDestroy(e->aux);
  if (e->word_index) (void)hipFree(e->word_index);
  delete e;
}
extern "C" size_t crct_engine_workspace_bytes(const crct_engine_t* e) { return e ? e->ws_bytes : 0; }
extern "C" int crct_engine_num_segments(const crct_engine_t* e) { return e ? (int)e->seg_range.size() : 0; }
extern "C" int crct_engine_segment_range(const crct_engine_t* e, int seg, int64_t* lo, int64_t* hi) {
  CRCT_REQUIRE(e && seg >= 0 && seg < (int)e->seg_range.size(), "segment_range: bad segment %d", seg);
  *lo = e->seg_range[seg].first; *hi = e->seg_range[seg].second;
  return 0;
}

namespace {

int ensure_streams(crct_engine* e, hipStream_t main) {
  // all internal streams share the caller's (default) priority: giving the weight-gradient streams the lowest or the
  // visual stream the highest priority (hipStreamCreateWithPriority) was measured to DOUBLE the step time on MI355X
  // (10.7 -> 21.9 ms, round 1) -- cross-priority event waits are slow -- so there is no priority knob
  if (!e->placed) {          // once per engine: streams on hardware queues that do not collide with the caller's or each other
    e->placed = true;
    e->placed_for = main;
    hipStream_t out[4];
    if (int r = crct_streams_place(main, out, &e->queue_classes)) return r;
    e->side[0] = out[0]; e->side[1] = out[1]; e->aux = out[2]; e->side[2] = out[3];
    // the word-table index (first / last row per token id) is the ENGINE's memory: it must be zero whenever a backward pass starts --
    // zeroed here once, kept zero by the kernels themselves (include/crct_hip.h) -- which a caller-provided workspace cannot promise
    const size_t index_bytes = (size_t)2 * e->d.vocab * sizeof(int32_t);
    if (hipMalloc((void**)&e->word_index, index_bytes) != hipSuccess) {
      e->word_index = nullptr;
      (void)hipGetLastError();
      crct_set_error("engine: cannot allocate the word index (%zu bytes)", index_bytes);
      return 1;
    }
    CRCT_CHECK_HIP(hipMemsetAsync(e->word_index, 0, index_bytes, main));
    CRCT_CHECK_HIP(hipStreamSynchronize(main));      // zero before any stream the backward may run on reads it
  }
  for (int k = 0; k < 3; ++k) {
    const bool need = k == 0 ? e->use_vis_stream : (e->use_wgrad_stream && !(k == 2 && e->one_wgrad_stream));
    if (need && !e->side[k] && hipStreamCreateWithFlags(&e->side[k], hipStreamNonBlocking) != hipSuccess) {
      crct_set_error("engine: cannot create an internal HIP stream");
      return 1;
    }
  }
  return 0;
}

// two drivers over one workspace: Rt = text stream on the caller's stream, Rv = visual stream
void make_runs(crct_engine* e, const float* p32, const void* p16, float* g32, void* ws, hipStream_t main, const CrctBatch* batch,
               const CrctStepCfg* cfg, Run& Rt, Run& Rv) {
  hipStream_t vis = e->use_vis_stream ? e->side[0] : main;
  Rt = Run{e, p32, (const bf16_t*)p16, g32, (char*)ws, main, batch, cfg, e->use_wgrad_stream ? e->side[1] : main,
           e->partials[0], e->colsum_part[0], e->colsum_part[2]};
  Rv = Run{e, p32, (const bf16_t*)p16, g32, (char*)ws, vis, batch, cfg, e->use_wgrad_stream ? e->side[e->one_wgrad_stream ? 1 : 2] : vis,
           e->partials[1], e->colsum_part[1], e->colsum_part[3]};
  Rt.sets[0] = &e->st; Rt.sets[1] = &e->st2;
  Rv.sets[0] = &e->sv; Rv.sets[1] = &e->sv2;
  Rt.which = 0; Rv.which = 1;
}

// the split-K ticket words of both data streams start every engine call at zero (an aborted launch must not poison the next)
int reset_tickets(crct_engine* e, void* ws, hipStream_t s) {
  bool any = false;
  for (int a = 1; a < CRCT_SITE_COUNT && !any; ++a)
    for (int k = 0; k < 2; ++k)
      for (int ph = 0; ph < 2; ++ph) any = any || e->policy[a][k][ph].split_k > 1;      // weight gradients are never split
  if (!any) return 0;
  CRCT_CHECK_HIP(hipMemsetAsync((char*)ws + e->sk_cnt[0], 0, (size_t)2 * e->sk_tickets * 4, s));
  return 0;
}

}  // namespace

extern "C" int crct_engine_forward(crct_engine_t* e, const float* params_f32, const void* params_bf16, const CrctBatch* batch,
                                   const CrctStepCfg* cfg, void* workspace, float* logits, float* reg, float* stats,
                                   crct_stream_t stream) {
  CRCT_REQUIRE(e && params_f32 && params_bf16 && cfg && workspace && logits && reg && stats, "engine_forward: null argument");
  if (int r = check_batch(e, batch)) return r;
  CRCT_REQUIRE(!cfg->fp8 || (e->feat && e->var.regressor == CRCT_REGRESSOR_PLOTQA),
               "engine_forward: the fp8 step is built for the PlotQA model only, not for the dvqa / figure_qa variants");
  if (int r = ensure_streams(e, (hipStream_t)stream)) return r;
  e->evnext = 0;
  e->fwd_r32 = cfg->residual_fp32 != 0;                   // (host state only: what crct_engine_sequence_outputs reads the rows as)
  CrctDeviceScope on_device;                              // every launch below runs on this thread and the device stays
  // key masks the caller did not supply are built here (one launch) and kept in the workspace for the backward pass
  CrctBatch bl = *batch;
  if (!bl.text_keymask || !bl.image_keymask) {
    uint8_t* kt = bl.text_keymask ? nullptr : (uint8_t*)workspace + e->km_t;
    uint8_t* kv = bl.image_keymask ? nullptr : (uint8_t*)workspace + e->km_v;
    if (int r = crct_build_keymasks(bl.sep_indices, bl.hist_len, bl.sep_stride, bl.image_mask, kt, kv, bl.B, bl.T, bl.V, stream)) return r;
    if (kt) bl.text_keymask = kt;
    if (kv) bl.image_keymask = kv;
  }
  batch = &bl;
  Run Rt, Rv;
  make_runs(e, params_f32, params_bf16, nullptr, workspace, (hipStream_t)stream, batch, cfg, Rt, Rv);
  if (int r = reset_tickets(e, workspace, (hipStream_t)stream)) return r;
  Rv.fail(order_streams(e, Rt.s, Rv.s));                 // fork: the visual stream starts after the caller's prior work
  // parameters of backward-segment `seg` may still be in the hands of an optimizer update running on another
  // stream (crct.optim overlap mode): wait for its event right before the first kernel that reads them
  const int nseg = (int)e->seg_range.size();
  auto wait_params = [&](Run& R, int seg) {
    if (!cfg->seg_ready_events || R.rc) return;
#ifdef CRCT_GEMM_LAB   // timing only: the forward does not wait for the overlapped optimizer update (reads parameters mid-update)
    static const bool lab_no_wait = getenv("CRCT_LAB_NO_PARAM_WAIT") != nullptr;
    if (lab_no_wait) return;
#endif
    hipEvent_t ev = (hipEvent_t)cfg->seg_ready_events[seg];
    if (ev && hipStreamWaitEvent(R.s, ev, 0) != hipSuccess) { crct_set_error("engine: wait on a parameter-ready event failed"); R.rc = 1; }
  };
  wait_params(Rt, nseg - 1);
  wait_params(Rv, nseg - 1);
  Rt.embed_text_fwd();
  Rv.embed_image_fwd();
  for (size_t i = 0; i < e->sched.size(); ++i) {
    const Step& st = e->sched[i];
    const StepIn& x = e->in[i];
    const int seg = (int)(e->sched.size() - i) + e->lm_seg;          // backward segment of this schedule step
    Rt.phase = (e->first_conn < 0 || (int)i < e->first_conn) ? 0 : 1;      // text-only prefix: nothing else on the data path
    if (st.kind != 'v') wait_params(Rt, seg);
    if (st.kind != 't') wait_params(Rv, seg);
    if (st.kind == 't') Rt.self_fwd(st.idx, x.t);
    else if (st.kind == 'v') Rv.self_fwd(st.idx, x.v);
    else Rt.conn_fwd(Rv, st.idx, x);
  }
  Rt.phase = 1;
  wait_params(Rt, e->lm_seg);
  wait_params(Rv, e->lm_seg);
  Rt.heads_branch_fwd(false, e->in.back().t.x);
  Rv.heads_branch_fwd(true, e->in.back().v.x);
  Rt.fail(order_streams(e, Rv.s, Rt.s));                 // join
  Rt.heads_tail_fwd(logits, reg, stats);
  return Rt.rc ? Rt.rc : Rv.rc;
}

extern "C" int crct_engine_backward(crct_engine_t* e, const float* params_f32, const void* params_bf16, const CrctBatch* batch,
                                    const CrctStepCfg* cfg, void* workspace, float* grads_f32, float* logits, float* reg,
                                    float* stats, int seg, crct_stream_t stream) {
  CRCT_REQUIRE(e && params_f32 && params_bf16 && cfg && workspace && grads_f32 && logits && reg && stats, "engine_backward: null argument");
  CRCT_REQUIRE(batch && batch->labels, "engine_backward: labels are required (training step)");
  if (int r = check_batch(e, batch)) return r;
  CRCT_REQUIRE(!e->req.ig.d_areas || e->areas, "engine_backward: d_areas is requested (crct_engine_set_input_grads) but the batch has no areas (crct_engine_set_areas)");
  CRCT_REQUIRE(e->req.amg.empty() || !cfg->fp8_bwd, "engine_backward: attention-map gradients are requested (crct_engine_set_attention_map_grads) with fp8_bwd=%d: "
               "the e5m2 copies of dqkv are written by the attention backward itself and would go stale", cfg->fp8_bwd);
  if (int r = ensure_streams(e, (hipStream_t)stream)) return r;
  e->evnext = 0;
  CrctDeviceScope on_device;                              // every launch below runs on this thread and the device stays
  CrctBatch bl = *batch;                                 // masks built by the forward pass of this batch live in the workspace
  if (!bl.text_keymask) bl.text_keymask = (const uint8_t*)workspace + e->km_t;
  if (!bl.image_keymask) bl.image_keymask = (const uint8_t*)workspace + e->km_v;
  batch = &bl;
  Run Rt, Rv;
  make_runs(e, params_f32, params_bf16, grads_f32, workspace, (hipStream_t)stream, batch, cfg, Rt, Rv);
  const int nseg = (int)e->seg_range.size();
  const int s0 = seg < 0 ? 0 : seg, s1 = seg < 0 ? nseg : seg + 1;
  CRCT_REQUIRE(s1 <= nseg, "engine_backward: bad segment %d", seg);
  if (s0 == 0) e->wgrad_pass_begin();
  if (seg >= 0 && !e->plan[seg].runs) return 0;          // nothing in or below this segment has a gradient: no launch, no event
  if (int r = reset_tickets(e, workspace, (hipStream_t)stream)) return r;
  // fork: every internal stream starts after the caller's prior work (previous segment, optimizer, ...)
  Rv.fail(order_streams(e, Rt.s, Rv.s));
  int ev_from = s0;                                      // segments enqueued completely but not yet marked for the data-parallel caller
  for (int sgi = s0; sgi < s1 && !Rt.rc && !Rv.rc; ++sgi) {
    const int hd = e->lm_seg;                            // the heads' segment (behind the masked-LM head's, which launches nothing here)
    const bool in_sched = sgi > hd && sgi != nseg - 1;
    const size_t si = in_sched ? e->sched.size() - (size_t)(sgi - hd) : 0;
    Rt.phase = (in_sched && (e->first_conn < 0 || (int)si < e->first_conn)) ? 0 : 1;      // backward tail through the text-only layers
    const SegPlan& pl = e->plan[sgi];
    if (!pl.runs) {
      // not run; its events below are still recorded, so a caller waiting on them never sees the previous pass's
    } else if (sgi < hd) {
      // the masked-LM head's segment: its gradients are in place
    } else if (sgi == hd) {
      e->cur_t = 0; e->cur_v = 0;
      Rt.heads_bwd(Rv, e->in.back().t.x, e->in.back().v.x, e->st.dy[0], e->sv.dy[0], logits, reg, stats);
    } else if (sgi == nseg - 1) {
      // each half: the parameter gradients where a tensor of the embedding has one -- the image half of 'plotqa' also for a requested
      // feature gradient, whose GEMM reads the bf16 d_sum that kernel stores -- then the requested input gradients on the same stream
      if (pl.dx_t && e->emb_own_t) Rt.embed_text_bwd(e->st.dy[e->cur_t]);
      if (pl.dx_t && e->req.ig_text()) Rt.embed_text_input_grads(e->st.dy[e->cur_t]);
      if (pl.dx_v && (e->emb_own_v || e->req.ig.d_image_feat)) Rv.embed_image_bwd(e->sv.dy[e->cur_v]);
      if (pl.dx_v && e->req.ig_vis()) Rv.embed_image_input_grads(e->sv.dy[e->cur_v]);
    } else {
      const Step& st = e->sched[si];
      const StepIn& x = e->in[si];
      const size_t gt = e->st.dy[e->cur_t], gxt = e->st.dy[e->cur_t ^ 1], gv = e->sv.dy[e->cur_v], gxv = e->sv.dy[e->cur_v ^ 1];
      if (st.kind == 't') Rt.self_bwd(st.idx, x.t, gt, gxt, pl.dx_t);
      else if (st.kind == 'v') Rv.self_bwd(st.idx, x.v, gv, gxv, pl.dx_v);
      else Rt.conn_bwd(Rv, st.idx, x, gv, gt, gxv, gxt, pl.dx_v, pl.dx_t);
      if (st.kind != 'v') e->cur_t ^= 1;
      if (st.kind != 't') e->cur_v ^= 1;
    }
    if (seg < 0 && cfg->seg_done_events && !Rt.rc && !Rv.rc) {
      // segments ev_from .. sgi are completely enqueued: mark that point on every internal stream for the data-parallel caller
      Rt.flush_wgrads();
      Rv.flush_wgrads();
      hipStream_t ss[4] = {Rt.s, Rt.sw, Rv.s, Rv.sw};
      for (int sg = ev_from; sg <= sgi; ++sg) {
        if (cfg->seg_done_mask && !cfg->seg_done_mask[sg]) continue;
        for (int k = 0; k < 4; ++k) {
          hipEvent_t ev = (hipEvent_t)cfg->seg_done_events[4 * sg + k];
          if (ev && hipEventRecord(ev, ss[k]) != hipSuccess) { crct_set_error("engine_backward: cannot record a segment event"); Rt.rc = 1; }
        }
        // the data-parallel caller launches the bucket this segment completes NOW, while the rest of backward is still being enqueued
        if (cfg->seg_enqueued && !Rt.rc) cfg->seg_enqueued(sg, cfg->seg_enqueued_user);
      }
    }
    ev_from = sgi + 1;
  }
  // join: everything this call enqueued anywhere is ordered before later work on the caller's stream
  Rt.main_after_wgrad();
  Rv.main_after_wgrad();
  Rt.fail(order_streams(e, Rv.s, Rt.s));
  return Rt.rc ? Rt.rc : Rv.rc;
}

extern "C" int crct_engine_wgrad_owned(crct_engine_t* e, int64_t* offsets, int64_t* numels, int cap) {
  if (!e) return -1;
  std::vector<std::pair<int64_t, int64_t>> v(e->wgrad_owned.begin(), e->wgrad_owned.end());
  std::sort(v.begin(), v.end());
  int n = 0;
  for (const auto& kv : v) {
    if (offsets && numels && n < cap) { offsets[n] = kv.first; numels[n] = kv.second; }
    ++n;
  }
  return n;
}

extern "C" int crct_engine_fp8_sites(const crct_engine_t* e) { return e ? e->n_sites : 0; }
extern "C" int crct_engine_fp8_grad_sites(const crct_engine_t* e) { return e ? e->n_gsites : 0; }
extern "C" int crct_engine_fp8_weights(const crct_engine_t* e, int64_t* offsets, int64_t* numels, int cap) {
  if (!e) return -1;
  const int n = (int)e->wq_list.size();
  for (int i = 0; i < n && i < cap && offsets && numels; ++i) { offsets[i] = e->wq_list[i].first; numels[i] = e->wq_list[i].second; }
  return n;
}

extern "C" int crct_engine_set_streams(crct_engine_t* e, int use_visual_stream, int use_wgrad_streams) {
  if (!e) return 1;
  e->use_vis_stream = use_visual_stream != 0;
  e->use_wgrad_stream = use_wgrad_streams != 0;
  e->one_wgrad_stream = use_wgrad_streams == 2;
  e->streams_forced = true;
  return 0;
}

// ---- device-scope ordering events for the host-side glue (optimizer overlap, data-parallel buckets): hipEventDisableTiming |
// hipEventDisableSystemFence, like the engine's internal ones.  A stock torch.cuda.Event carries a system-scope fence (host /
// peer visibility) in every record, which these same-device stream orderings do not need.
extern "C" void* crct_event_create(void) {
  hipEvent_t ev = nullptr;
  const unsigned flags = hipEventDisableTiming | hipEventDisableSystemFence;
  if (hipEventCreateWithFlags(&ev, flags) != hipSuccess) { crct_set_error("event_create: hipEventCreateWithFlags failed"); return nullptr; }
  return ev;
}
extern "C" void crct_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
extern "C" int crct_event_record(void* ev, crct_stream_t stream) {
  CRCT_REQUIRE(ev, "event_record: null event");
  CRCT_CHECK_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return 0;
}
extern "C" int crct_stream_wait_event(crct_stream_t stream, void* ev) {
  CRCT_REQUIRE(ev, "stream_wait_event: null event");
  CRCT_CHECK_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
  return 0;
}
extern "C" int crct_event_query(void* ev) {          // 1: everything before the last record has finished, 0: not yet, < 0: error
  if (!ev) return -1;
  const hipError_t r = hipEventQuery((hipEvent_t)ev);
  if (r == hipSuccess) return 1;
  if (r == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
  crct_set_error("event_query: %s", hipGetErrorString(r));
  return -1;
}
extern "C" int crct_event_synchronize(void* ev) {
  CRCT_REQUIRE(ev, "event_synchronize: null event");
  CRCT_CHECK_HIP(hipEventSynchronize((hipEvent_t)ev));
  return 0;
}

extern "C" crct_stream_t crct_engine_aux_stream(crct_engine_t* e, crct_stream_t main_stream, int* queue_classes) {
  if (!e) return nullptr;
  if (ensure_streams(e, (hipStream_t)main_stream)) return nullptr;
  if (queue_classes) *queue_classes = e->queue_classes;
  return e->aux;
}

extern "C" int crct_engine_streams(crct_engine_t* e, crct_stream_t out[4]) {
  if (!e || !out) return 1;
  out[0] = e->side[0]; out[1] = e->side[1]; out[2] = e->side[2]; out[3] = e->aux;
  return 0;
}

extern "C" int crct_engine_set_wgrad_workgroups(crct_engine_t* e, int target_wgs, int max_rows) {
  if (!e) return 1;
  e->wgrad_target = target_wgs > 0 ? target_wgs : 0;
  e->wgrad_target_rows = max_rows;
  return 0;
}
extern "C" int crct_engine_set_wgrad_flush(crct_engine_t* e, int mode) {
  if (!e) return 1;
  e->wgrad_flush = mode;
  return 0;
}

extern "C" int crct_engine_set_ln_addend(crct_engine_t* e, int on) {
  if (!e) return 1;
  e->ln_addend = on != 0;
  e->ws_update();
  return 0;
}

extern "C" int crct_engine_set_site_policy(crct_engine_t* e, int site, int kind, int phase, int cfg, int split_k) {
  CRCT_REQUIRE(e && site > 0 && site < CRCT_SITE_COUNT && kind >= CRCT_KIND_FWD && kind <= CRCT_KIND_WGRAD && phase <= 1,
               "set_site_policy: bad site / kind / phase (%d, %d, %d)", site, kind, phase);
  CRCT_REQUIRE(cfg == -1 || crct_gemm_config_built(cfg), "set_site_policy: configuration %d is not built", cfg);
  CRCT_REQUIRE(split_k >= 0 && split_k <= 4, "set_site_policy: split_k %d out of range", split_k);
  for (int ph = 0; ph < 2; ++ph)
    if (phase < 0 || phase == ph) { e->policy[site][kind][ph].cfg = cfg; e->policy[site][kind][ph].split_k = split_k; }
  return 0;
}

extern "C" int64_t crct_engine_tap(crct_engine_t* e, const void* workspace, const char* name, int B, int T, int V, void* out,
                                   int64_t cap, crct_stream_t stream) {
  if (!e || !name) return -1;
  auto copy = [&](const Tap& t) -> int64_t {
    const int64_t n = t.stream == 't' ? (int64_t)B * T * (t.width ? t.width : e->d.H) : (int64_t)B * V * (t.width ? t.width : e->d.Hv);
    if (n > cap) { crct_set_error("tap: buffer too small"); return -1; }
    if (hipMemcpyAsync(out, (const char*)workspace + t.off, (size_t)n * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return -1;
    return n;
  };
  // the running hidden gradients, resolved at call time: the buffers the next backward segment reads
  if (!strcmp(name, "grad.t")) return copy(Tap{name, e->st.dy[e->cur_t], 't'});
  if (!strcmp(name, "grad.v")) return copy(Tap{name, e->sv.dy[e->cur_v], 'v'});
  for (const Tap& t : e->taps)
    if (t.name == name) return copy(t);
  crct_set_error("tap: unknown activation '%s'", name);
  return -1;
}

extern "C" int64_t crct_engine_attention_probs(crct_engine_t* e, const CrctBatch* batch, const CrctStepCfg* cfg, const void* workspace, int kind,
                                               int index, int direction, float* out, int64_t cap, crct_stream_t stream) {
  if (!e || !cfg || !workspace || !out) { crct_set_error("engine_attention_probs: null argument"); return -1; }
  if (check_batch(e, batch)) return -1;
  AttnSite a;
  if (e->attn_site("engine_attention_probs", kind, index, direction, batch->T, batch->V, &a)) return -1;
  const char* ws = (const char*)workspace;
  // the key mask as crct_engine_backward resolves it: the caller's, else the one the forward built in the workspace
  const uint8_t* km = a.image_keys ? (batch->image_keymask ? batch->image_keymask : (const uint8_t*)ws + e->km_v)
                                   : (batch->text_keymask ? batch->text_keymask : (const uint8_t*)ws + e->km_t);
  const int64_t n = (int64_t)batch->B * a.heads * a.Tq * a.Tk;
  if (n > cap) { crct_set_error("engine_attention_probs: %lld elements do not fit the buffer of %lld", (long long)n, (long long)cap); return -1; }
  const Drop dr = drop_of(cfg, a.p, a.site);
  if (crct_attention_probs((const bf16_t*)(ws + a.q), (const bf16_t*)(ws + a.k), km, out, batch->B, a.heads, a.Tq, a.Tk, a.d, a.ld, a.ld, dr.thr, dr.scale,
                           dr.site, cfg->seed, stream)) return -1;
  return n;
}
