// Classification head + regression tail + joint loss, and their gradient seeds, without host syncs.
// Reference: BertPreTrainingHeads.forward vilbert.py:1048-1062 (fusion 'mul'/'sum', dropout 0.1,
// Linear(1024, 2)); PlotQA_Regressor_v20 tail regressor.py:31-34,41 (Linear(256,1) + Tanh);
// regression bookkeeping + CrossEntropyLoss(ignore_index=-1) vilbert.py:1583-1657; loss
// combination encoder_decorator.py:144-153.  All B rows are regressed and masked by R[:,1]
// (the reference gathers those rows: same values, same gradients, static shapes).
#include "common.hip.h"
#include "crct_internal.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ bool head_keep(const CrctHeadArgs& a, int b, int c) {
  if (!a.drop_thr) return true;
  const uint64_t idx = (uint64_t)b * (uint64_t)a.Hb + (uint64_t)c;
  return (philox_keep8(a.seed, a.drop_site, idx >> 3, a.drop_thr) >> ((uint32_t)idx & 7u)) & 1u;
}

// values of the variants' regressors (CrctVariant), passed by value
struct HeadValues { float v[CRCT_CE_CLASSES]; int n; };

// the PlotQA regressor's tail: MODE 0 = PlotQA, 1 = DVQA evaluation snap (vilbert.py:1619-1625), 2 = no regressor
enum { HEAD_PLOTQA = 0, HEAD_SNAP = 1, HEAD_NONE = 2 };

// scratch row layout (fp32 x 8): dlogit0, dlogit1, dz, nsp_loss_b, valid, ok5, okt, needs
// sg: upstream gradients of the logits and of the regressed value reg[0] (CrctScoreGrads, members NULL = none): added to dlogit0 / dlogit1
// and dz before anything is formed from them, so every gradient below carries them with the one rounding it always had
template <int MODE>
__global__ __launch_bounds__(256) void head_rows_kernel(const CrctHeadArgs a, float* scratch, const HeadValues hv, const CrctScoreGrads sg) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const bf16_t* pt = reinterpret_cast<const bf16_t*>(a.pooled_t) + (long)b * a.Hb;
  const bf16_t* pv = reinterpret_cast<const bf16_t*>(a.pooled_v) + (long)b * a.Hb;
  const bf16_t* fh = reinterpret_cast<const bf16_t*>(a.fus_h) + (long)b * 256;
  const float dsc = a.drop_thr ? a.drop_scale : 1.0f;
  // ---- logits
  float l0 = 0.f, l1 = 0.f;
  for (int c = tid; c < a.Hb; c += 256) {
    const float t = bf2f(pt[c]), v = bf2f(pv[c]);
    float f = a.fusion_sum ? t + v : t * v;
    f = head_keep(a, b, c) ? f * dsc : 0.f;
    l0 += f * a.w_cls[c]; l1 += f * a.w_cls[a.Hb + c];
  }
  l0 = block_sum(l0, red) + a.b_cls[0];
  l1 = block_sum(l1, red) + a.b_cls[1];
  // ---- regression tail
  float z = 0.f;
  if (MODE != HEAD_NONE) {
    for (int c = tid; c < 256; c += 256) z += bf2f(fh[c]) * a.w_f6[c];
    z = block_sum(z, red) + a.b_f6[0];
  }
  float r = tanhf(z);
  // ---- labels: count of rows that enter the CE mean (ignore_index = -1)
  int n_valid = 0;
  long label = -1;
  if (a.labels) {
    for (int i = tid; i < a.B; i += 256) n_valid += (a.labels[i] != -1);
    n_valid = (int)(block_sum((float)n_valid, red) + 0.5f);
    label = a.labels[b];
  }
  // upstream gradients of the two differentiable outputs (nsp_loss scalar, reg_loss rows): either
  // device tensors handed over by autograd, or the fixed combination of encoder_decorator.py:144-153
  // g_loss_dev: upstream gradient of the COMBINED loss stats[0] (a device scalar: 1, 1 / batch_multiply, a GradScaler scale ...)
  const float g_loss = (a.g_loss_dev ? a.g_loss_dev[0] : 1.0f) * a.grad_scale;
  const float g_nsp = a.g_nsp_dev ? a.g_nsp_dev[0] * a.grad_scale : a.nsp_coeff * g_loss;
  const float g_reg = a.g_reg_dev ? a.g_reg_dev[b] * a.grad_scale : a.reg_coeff * g_loss / (float)a.B;
  // per-row scalars (every thread computes them identically)
  const float mx = fmaxf(l0, l1);
  const float lse = mx + logf(expf(l0 - mx) + expf(l1 - mx));
  float nsp_b = 0.f, dl0 = 0.f, dl1 = 0.f;
  const bool valid = a.labels && label != -1;
  if (valid) {
    nsp_b = lse - (label == 0 ? l0 : l1);
    const float w = g_nsp / (float)max(n_valid, 1);
    dl0 = (expf(l0 - lse) - (label == 0 ? 1.f : 0.f)) * w;
    dl1 = (expf(l1 - lse) - (label == 1 ? 1.f : 0.f)) * w;
  }
  if (sg.d_logits) {                       // every row, label -1 included: the logits are outputs whatever the label says
    dl0 += a.grad_scale * sg.d_logits[b * 2]; dl1 += a.grad_scale * sg.d_logits[b * 2 + 1];
  }
  const float* Rb = a.R + (long)b * 4;
  const bool needs = Rb[1] == 1.0f;
  const float target = Rb[0] / Rb[3];
  const float raw = r;
  if (MODE == HEAD_SNAP && needs) {       // nearest table value of r * scale (first on a tie), divided back
    // x is the ROUNDED product for every entry: contracted into the subtraction (fma(-r, scale, v[0])), entry 0 alone was measured
    // from the unrounded product and lost or won exact ties against the others by that rounding
#pragma clang fp contract(off)
    const float x = r * Rb[3];
    float best = hv.v[0], bd = fabsf(hv.v[0] - x);
    for (int k = 1; k < hv.n; ++k) {
      const float d = fabsf(hv.v[k] - x);
      if (d < bd) { bd = d; best = hv.v[k]; }
    }
    r = best / Rb[3];
  }
  const float diff = r - target, l1v = fabsf(diff);
  float rl, drl;   // reg loss and d(reg loss)/dr
  if (a.use_l1) { rl = l1v; drl = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f); }
  else {           // SmoothL1, beta = 0.5
    if (l1v < 0.5f) { rl = diff * diff; drl = 2.0f * diff; }    // 0.5 d^2 / beta
    else { rl = l1v - 0.25f; drl = diff > 0.f ? 1.f : -1.f; }
  }
  const bool both0 = (r == 0.f) && (target == 0.f);
  float d5 = l1v / fabsf(target);
  if (target == 0.f) d5 = 1.f;
  if (both0) d5 = 0.f;
  const bool ok5 = ((d5 <= 0.05f) || both0) && needs;
  const bool okt = (l1v <= a.tol_margin) && needs;
  if (!a.kind_l1 && fabsf(target) > 1.f) { rl = 0.f; drl = 0.f; }
  if (!needs) { rl = 0.f; drl = 0.f; }
  if (MODE == HEAD_SNAP) drl = 0.f;       // the snapped value is a constant
  float dz = drl * g_reg * (1.f - r * r);
  // reg[0] = r * R[:,3] on the needs rows: its upstream passes the tanh whatever the loss rules above zeroed; the snapped value is a constant
  if (MODE == HEAD_PLOTQA && sg.d_value && needs) dz += a.grad_scale * sg.d_value[b] * Rb[3] * (1.f - r * r);
  if (MODE == HEAD_NONE) {                // no regressor module: reg rows stay zero (vilbert.py:1592-1598)
    if (tid == 0) {
      a.logits[b * 2] = l0; a.logits[b * 2 + 1] = l1;
      for (int k = 0; k < 5; ++k) a.reg[k * a.B + b] = 0.f;
      float* s = scratch + (long)b * 8;
      s[0] = dl0; s[1] = dl1; s[2] = 0.f; s[3] = nsp_b; s[4] = valid ? 1.f : 0.f;
      s[5] = 0.f; s[6] = 0.f; s[7] = needs ? 1.f : 0.f;
    }
  } else
  if (tid == 0) {
    a.logits[b * 2] = l0; a.logits[b * 2 + 1] = l1;
    a.reg[0 * a.B + b] = needs ? r * Rb[3] : 0.f;
    a.reg[1 * a.B + b] = rl;
    a.reg[2 * a.B + b] = needs ? l1v : 0.f;
    a.reg[3 * a.B + b] = raw;                     // raw tanh output (diagnostic)
    a.reg[4 * a.B + b] = needs ? d5 : 0.f;
    float* s = scratch + (long)b * 8;
    s[0] = dl0; s[1] = dl1; s[2] = dz; s[3] = nsp_b; s[4] = valid ? 1.f : 0.f;
    s[5] = ok5 ? 1.f : 0.f; s[6] = okt ? 1.f : 0.f; s[7] = needs ? 1.f : 0.f;
  }
  // ---- gradient seeds (w.r.t. the PRE-activations of the poolers / fusion.4)
  if (a.d_pooled_t) {
    bf16_t* dpt = reinterpret_cast<bf16_t*>(a.d_pooled_t) + (long)b * a.Hb;
    bf16_t* dpv = reinterpret_cast<bf16_t*>(a.d_pooled_v) + (long)b * a.Hb;
    for (int c = tid; c < a.Hb; c += 256) {
      const float t = bf2f(pt[c]), v = bf2f(pv[c]);
      float df = dl0 * a.w_cls[c] + dl1 * a.w_cls[a.Hb + c];
      df = head_keep(a, b, c) ? df * dsc : 0.f;
      const float gt = a.fusion_sum ? df : df * v, gv = a.fusion_sum ? df : df * t;
      dpt[c] = f2bf(t <= 0.f ? 0.f : gt);       // relu'(pre) == (post > 0); a NaN post lets the gradient through, as torch's threshold_backward does
      dpv[c] = f2bf(v <= 0.f ? 0.f : gv);
    }
    if (MODE != HEAD_NONE) {
      bf16_t* dfh = reinterpret_cast<bf16_t*>(a.d_fus_h) + (long)b * 256;
      for (int c = tid; c < 256; c += 256) {
        const float hval = bf2f(fh[c]);
        dfh[c] = f2bf(dz * a.w_f6[c] * (hval > 0.f ? 1.f : 0.01f));
      }
    }
  }
}

// stats + parameter gradients of bi_seq_relationship and fusion.6 (sums over the batch rows)
__global__ __launch_bounds__(256) void head_reduce_kernel(const CrctHeadArgs a, const float* scratch) {
  const int tid = threadIdx.x;
  const float dsc = a.drop_thr ? a.drop_scale : 1.0f;
  // parameter gradients: 32 columns x 8 row groups per workgroup (a thread walks B / 8 rows, not all of them), the 8
  // partial sums are added in a fixed order.  Columns beyond Hb / 256 idle.
  __shared__ float part[3][8][33];
  const int cl = tid & 31, rg = tid >> 5;
  const int cc = blockIdx.x * 32 + cl;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  if (a.d_w_cls && cc < a.Hb) {
    const bf16_t* pt = reinterpret_cast<const bf16_t*>(a.pooled_t);
    const bf16_t* pv = reinterpret_cast<const bf16_t*>(a.pooled_v);
    for (int b = rg; b < a.B; b += 8) {
      const float t = bf2f(pt[(long)b * a.Hb + cc]), v = bf2f(pv[(long)b * a.Hb + cc]);
      float f = a.fusion_sum ? t + v : t * v;
      f = head_keep(a, b, cc) ? f * dsc : 0.f;
      g0 += scratch[b * 8] * f; g1 += scratch[b * 8 + 1] * f;
    }
  }
  if (a.d_w_f6 && cc < 256) {
    const bf16_t* fh = reinterpret_cast<const bf16_t*>(a.fus_h);
    for (int b = rg; b < a.B; b += 8) g2 += scratch[b * 8 + 2] * bf2f(fh[(long)b * 256 + cc]);
  }
  part[0][rg][cl] = g0; part[1][rg][cl] = g1; part[2][rg][cl] = g2;
  __syncthreads();
  if (rg == 0) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { t0 += part[0][k][cl]; t1 += part[1][k][cl]; t2 += part[2][k][cl]; }
    if (a.d_w_cls && cc < a.Hb) { a.d_w_cls[cc] += t0; a.d_w_cls[a.Hb + cc] += t1; }
    if (a.d_w_f6 && cc < 256) a.d_w_f6[cc] += t2;
  }
  if (blockIdx.x == 0 && tid < 64) {
    // one wave reduces the per-row records
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float rl = 0.f, d5 = 0.f;
    for (int b = tid; b < a.B; b += 64) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += scratch[b * 8 + k];
      rl += a.reg[1 * a.B + b];
      d5 += a.reg[4 * a.B + b];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = wave_sum(s[k]);
    rl = wave_sum(rl);
    d5 = wave_sum(d5);
    if (tid == 0) {
      const float nsp = s[4] > 0.f ? s[3] / s[4] : 0.f;
      const float reg_mean = rl / (float)a.B;
      a.stats[0] = a.labels ? a.nsp_coeff * nsp + a.reg_coeff * reg_mean : 0.f;
      a.stats[1] = nsp; a.stats[2] = reg_mean; a.stats[3] = s[7]; a.stats[4] = s[5]; a.stats[5] = s[6];
      a.stats[6] = s[4]; a.stats[7] = 0.f;
      // stats[8..16]: the 9 floats train.py:181-183 shares between the ranks every iteration, ready for the all-reduce
      // (loss, lm_loss = 0, nsp_loss, mean reg_loss / mean reg_5_dist over the rows that need regression -- 0 when there
      // are none, as the reference's isnan test does --, legend_loss = 0, num_regs, reg_5_right, reg_t_right)
      a.stats[8] = a.stats[0]; a.stats[9] = 0.f; a.stats[10] = nsp;
      a.stats[11] = s[7] > 0.f ? rl / s[7] : 0.f; a.stats[12] = s[7] > 0.f ? d5 / s[7] : 0.f; a.stats[13] = 0.f;
      a.stats[14] = s[7]; a.stats[15] = s[5]; a.stats[16] = s[6];
      if (a.d_b_cls) { a.d_b_cls[0] += s[0]; a.d_b_cls[1] += s[1]; }
      if (a.d_b_f6) a.d_b_f6[0] += s[2];
    }
  }
}

// ------------------------------------------------------------------ DVQA_Regressor_v20_CE tail
// regressor.py:72-79 + vilbert.py:1603-1615.  One workgroup per row: logits / NSP terms as head_rows_kernel, z = ce_fusion.6(fus_h)
// (65 outputs, the four waves take them in turn), p = softmax(z), CrossEntropyLoss(p, target) -- the reference feeds the Softmax
// output to CrossEntropyLoss, so the softmax is taken twice -- argmax (first maximum), value lookup and flags.  Writes the gradient
// seed w.r.t. ce_fusion.4's pre-activation and the per-row dL/dz (ce [B][65]) for the weight gradients of ce_fusion.6.
__global__ __launch_bounds__(256) void head_ce_rows_kernel(const CrctHeadArgs a, float* scratch, float* ce, const HeadValues hv,
                                                           const CrctScoreGrads sg) {
  __shared__ float red[4];
  __shared__ float zs[CRCT_CE_CLASSES], ps[CRCT_CE_CLASSES], dzs[CRCT_CE_CLASSES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* pt = reinterpret_cast<const bf16_t*>(a.pooled_t) + (long)b * a.Hb;
  const bf16_t* pv = reinterpret_cast<const bf16_t*>(a.pooled_v) + (long)b * a.Hb;
  const bf16_t* fh = reinterpret_cast<const bf16_t*>(a.fus_h) + (long)b * 256;
  const float dsc = a.drop_thr ? a.drop_scale : 1.0f;
  float l0 = 0.f, l1 = 0.f;
  for (int c = tid; c < a.Hb; c += 256) {
    const float t = bf2f(pt[c]), v = bf2f(pv[c]);
    float f = a.fusion_sum ? t + v : t * v;
    f = head_keep(a, b, c) ? f * dsc : 0.f;
    l0 += f * a.w_cls[c]; l1 += f * a.w_cls[a.Hb + c];
  }
  l0 = block_sum(l0, red) + a.b_cls[0];
  l1 = block_sum(l1, red) + a.b_cls[1];
  int n_valid = 0;
  long label = -1;
  if (a.labels) {
    for (int i = tid; i < a.B; i += 256) n_valid += (a.labels[i] != -1);
    n_valid = (int)(block_sum((float)n_valid, red) + 0.5f);
    label = a.labels[b];
  }
  for (int k = wave; k < CRCT_CE_CLASSES; k += 4) {
    float acc = 0.f;
    for (int c = lane; c < 256; c += 64) acc += bf2f(fh[c]) * a.w_f6[(long)k * 256 + c];
    acc = wave_sum(acc);
    if (lane == 0) zs[k] = acc + a.b_f6[k];
  }
  __syncthreads();
  const float g_loss = (a.g_loss_dev ? a.g_loss_dev[0] : 1.0f) * a.grad_scale;
  const float g_nsp = a.g_nsp_dev ? a.g_nsp_dev[0] * a.grad_scale : a.nsp_coeff * g_loss;
  const float g_reg = a.g_reg_dev ? a.g_reg_dev[b] * a.grad_scale : a.reg_coeff * g_loss / (float)a.B;
  const float mx = fmaxf(l0, l1);
  const float lse = mx + logf(expf(l0 - mx) + expf(l1 - mx));
  float nsp_b = 0.f, dl0 = 0.f, dl1 = 0.f;
  const bool valid = a.labels && label != -1;
  if (valid) {
    nsp_b = lse - (label == 0 ? l0 : l1);
    const float w = g_nsp / (float)max(n_valid, 1);
    dl0 = (expf(l0 - lse) - (label == 0 ? 1.f : 0.f)) * w;
    dl1 = (expf(l1 - lse) - (label == 1 ? 1.f : 0.f)) * w;
  }
  if (sg.d_logits) {                       // every row, label -1 included: the logits are outputs whatever the label says
    dl0 += a.grad_scale * sg.d_logits[b * 2]; dl1 += a.grad_scale * sg.d_logits[b * 2 + 1];
  }
  // p = softmax(z)
  float zm = zs[0];
  for (int k = 1; k < CRCT_CE_CLASSES; ++k) zm = fmaxf(zm, zs[k]);
  float se = 0.f;
  for (int k = 0; k < CRCT_CE_CLASSES; ++k) se += expf(zs[k] - zm);
  if (tid < CRCT_CE_CLASSES) ps[tid] = expf(zs[tid] - zm) / se;
  __syncthreads();
  // CrossEntropyLoss over p, argmax of p
  const float* Rb = a.R + (long)b * 4;
  const bool needs = Rb[1] == 1.0f;
  const float tf = Rb[0];
  const bool tok = tf > -1.f && tf < (float)CRCT_CE_CLASSES;      // (int64) R[:,0] truncates towards zero
  const int t = tok ? (int)tf : 0;
  int am = 0;
  float pm = ps[0];
  for (int k = 1; k < CRCT_CE_CLASSES; ++k) if (ps[k] > pm) { pm = ps[k]; am = k; }
  float s2 = 0.f;
  for (int k = 0; k < CRCT_CE_CLASSES; ++k) s2 += expf(ps[k] - pm);
  const float lse2 = pm + logf(s2);
  float pdp = 0.f;                                                   // sum_j p_j dL/dp_j
  for (int k = 0; k < CRCT_CE_CLASSES; ++k) pdp += ps[k] * (expf(ps[k] - lse2) - (k == t ? 1.f : 0.f));
  const float w = (needs && tok) ? g_reg : 0.f;
  if (tid < CRCT_CE_CLASSES) {
    const float dp = expf(ps[tid] - lse2) - (tid == t ? 1.f : 0.f);
    const float dz = w * ps[tid] * (dp - pdp);
    dzs[tid] = dz;
    if (ce) ce[(long)b * CRCT_CE_CLASSES + tid] = dz;
  }
  const float rl = needs ? (tok ? lse2 - ps[t] : NAN) : 0.f;
  const float err = (needs && tok) ? fabsf(hv.v[am] - hv.v[t]) : 0.f;
  const bool ok = needs && tok && am == t;
  if (tid == 0) {
    a.logits[b * 2] = l0; a.logits[b * 2 + 1] = l1;
    a.reg[0 * a.B + b] = needs ? hv.v[am] : 0.f;
    a.reg[1 * a.B + b] = rl;
    a.reg[2 * a.B + b] = err;
    a.reg[3 * a.B + b] = pm;                      // probability of the chosen class (diagnostic)
    a.reg[4 * a.B + b] = err;
    float* s = scratch + (long)b * 8;
    s[0] = dl0; s[1] = dl1; s[2] = 0.f; s[3] = nsp_b; s[4] = valid ? 1.f : 0.f;
    s[5] = ok ? 1.f : 0.f; s[6] = ok ? 1.f : 0.f; s[7] = needs ? 1.f : 0.f;
  }
  if (a.d_pooled_t) {
    __syncthreads();                              // dzs complete
    bf16_t* dpt = reinterpret_cast<bf16_t*>(a.d_pooled_t) + (long)b * a.Hb;
    bf16_t* dpv = reinterpret_cast<bf16_t*>(a.d_pooled_v) + (long)b * a.Hb;
    for (int c = tid; c < a.Hb; c += 256) {
      const float tv = bf2f(pt[c]), v = bf2f(pv[c]);
      float df = dl0 * a.w_cls[c] + dl1 * a.w_cls[a.Hb + c];
      df = head_keep(a, b, c) ? df * dsc : 0.f;
      const float gt = a.fusion_sum ? df : df * v, gv = a.fusion_sum ? df : df * tv;
      dpt[c] = f2bf(tv <= 0.f ? 0.f : gt);
      dpv[c] = f2bf(v <= 0.f ? 0.f : gv);
    }
    bf16_t* dfh = reinterpret_cast<bf16_t*>(a.d_fus_h) + (long)b * 256;
    for (int c = tid; c < 256; c += 256) {
      float g = 0.f;
      for (int k = 0; k < CRCT_CE_CLASSES; ++k) g += dzs[k] * a.w_f6[(long)k * 256 + c];
      const float hval = bf2f(fh[c]);
      dfh[c] = f2bf(g * (hval > 0.f ? 1.f : 0.01f));
    }
  }
}

// ce_fusion.6 gradients: d_w[k][c] += sum_b dz[b][k] fus_h[b][c], d_b[k] += sum_b dz[b][k]; one workgroup per class, rows in order
__global__ __launch_bounds__(256) void head_ce_wgrad_kernel(const CrctHeadArgs a, const float* __restrict__ ce) {
  const int k = blockIdx.x, c = threadIdx.x;
  const bf16_t* fh = reinterpret_cast<const bf16_t*>(a.fus_h);
  float g = 0.f, gb = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float d = ce[(long)b * CRCT_CE_CLASSES + k];
    g += d * bf2f(fh[(long)b * 256 + c]);
    gb += d;
  }
  a.d_w_f6[(long)k * 256 + c] += g;
  if (c == 0 && a.d_b_f6) a.d_b_f6[k] += gb;
}

// ------------------------------------------------------------------ evaluation: per-question answer selection
// One wave per question.  Question q owns the candidate rows [off_q, off_q + num_ans[q]) with off_q = sum of the
// earlier counts (recomputed by every wave: Q is a few hundred at most).  p0 = softmax(logits)[0] in fp32; the
// answer is the FIRST row with the largest p0 (torch.argmax), or forced[q] when given; the regressed value and its
// two error measures are gathered from the chosen row.  A NaN p0 is the maximum, as it is for torch.argmax: the first
// NaN row of a question wins over every number and over every later NaN.
// softmax(l0, l1)[0] in fp32: the one expression both evaluation kernels use
__device__ __forceinline__ float eval_p0(float l0, float l1) {
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  return e0 / (e0 + e1);
}

// what a question's wave picked: the answer, its row, and whether that row exists (0 <= a < num_ans[q] and r < N)
struct EvalPick { long a, r; bool ok; };

// The selection of one question by its wave (all 64 lanes call it; every lane returns the same pick).
__device__ __forceinline__ EvalPick eval_select_wave(const float* __restrict__ logits, const int64_t* __restrict__ num_ans,
                                                     const int64_t* __restrict__ forced, int q, int lane, long N,
                                                     float* __restrict__ prob0) {
  long off = 0;
  for (int i = lane; i < q; i += 64) off += num_ans[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
  const long n = num_ans[q];
  float best = -INFINITY;
  long best_i = 0x7fffffffffffffffL;
  for (long j = lane; j < n; j += 64) {
    const long r = off + j;
    float p = 0.f;
    if (r < N) {
      p = eval_p0(logits[2 * r], logits[2 * r + 1]);
      if (prob0) prob0[r] = p;
    }
    // strictly greater: the earliest row of this lane wins ties; a NaN replaces any number and is never replaced
    if (p > best || (p != p && best == best)) { best = p; best_i = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const long oi = __shfl_xor(best_i, o, 64);
    const bool on = ob != ob, bn = best != best;
    const bool take = on ? (!bn || oi < best_i) : (!bn && (ob > best || (ob == best && oi < best_i)));
    if (take) { best = ob; best_i = oi; }
  }
  EvalPick k;
  k.a = forced ? forced[q] : (n > 0 ? best_i : 0);
  k.r = off + k.a;
  k.ok = k.a >= 0 && k.a < n && k.r < N;
  return k;
}

__global__ __launch_bounds__(64) void eval_select_kernel(const float* __restrict__ logits, const float* __restrict__ reg_out,
                                                         const float* __restrict__ reg_err, const float* __restrict__ reg_terr,
                                                         const int64_t* __restrict__ num_ans, const int64_t* __restrict__ forced,
                                                         int Q, long N, float* __restrict__ prob0, int64_t* __restrict__ answers,
                                                         float* __restrict__ sel_out, float* __restrict__ sel_err,
                                                         float* __restrict__ sel_terr) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const EvalPick k = eval_select_wave(logits, num_ans, forced, q, lane, N, prob0);
  if (lane == 0) {
    answers[q] = k.a;
    sel_out[q] = k.ok ? reg_out[k.r] : 0.f;
    sel_err[q] = k.ok ? reg_err[k.r] : INFINITY;
    sel_terr[q] = k.ok ? reg_terr[k.r] : INFINITY;
  }
}

// ------------------------------------------------------------------ evaluation: selection, flags and the accuracy tables in one launch
// One wave per question, as above.  Mode 0 selects with eval_select_wave (the same bits as eval_select_kernel); mode 1 is the
// reference's binary_answers branch (evaluation.py:280-285): one row per question, answer = round-half-even(p0), right when it
// equals 1 - label.  Lane 0 then derives the flags (:303-311) and adds the question into tables (CRCT_EVAL_* offsets): 64-bit
// integer atomics only, so the sums are exact and do not depend on the order the waves arrive in.
__device__ __forceinline__ void eval_add(int64_t* tables, int i, bool on) {
  if (on) atomicAdd(reinterpret_cast<unsigned long long*>(tables) + i, 1ULL);
}

__global__ __launch_bounds__(64) void eval_score_kernel(const CrctEvalScoreArgs a) {
  const int q = blockIdx.x, lane = threadIdx.x;
  long ans;
  float so = 0.f, se = 0.f, st = 0.f;
  bool nsp_right;
  if (a.mode == 0) {
    const EvalPick k = eval_select_wave(a.logits, a.num_ans, a.forced, q, lane, a.N, a.prob0);
    if (lane != 0) return;
    ans = k.a;
    so = k.ok ? a.reg_out[k.r] : 0.f;
    se = k.ok ? a.reg_err[k.r] : INFINITY;
    st = k.ok ? a.reg_terr[k.r] : INFINITY;
    nsp_right = ans == a.gt_id[q];
  } else {
    if (lane != 0) return;
    const float p = eval_p0(a.logits[2 * (long)q], a.logits[2 * (long)q + 1]);
    if (a.prob0) a.prob0[q] = p;
    const bool nan = p != p;
    ans = nan ? -1 : (long)rintf(p);                  // round half to even, as torch.round / np.round: p0 = 0.5 answers 0
    nsp_right = !nan && ans == 1 - a.labels[q];
  }
  const bool needs = a.needs_reg[q] != 0;
  const bool reg_right = se <= 0.05f && needs;
  const bool reg_t_right = st <= a.tolerance[q] && needs;
  const bool correct = nsp_right && (!needs || reg_right), correct_t = nsp_right && (!needs || reg_t_right);
  a.answers[q] = ans;
  if (a.sel_out) a.sel_out[q] = so;
  if (a.sel_err) a.sel_err[q] = se;
  if (a.sel_terr) a.sel_terr[q] = st;
  if (a.flags) a.flags[q] = (uint8_t)((nsp_right ? 1 : 0) | (reg_right ? 2 : 0) | (reg_t_right ? 4 : 0));
  int64_t* total = a.tables + CRCT_EVAL_TOTAL;       // [6][2] (hits, count), evaluation.py:492-519
  eval_add(total, 0, nsp_right);            eval_add(total, 1, true);
  eval_add(total, 2, nsp_right && needs);   eval_add(total, 3, needs);
  eval_add(total, 4, reg_right);            eval_add(total, 5, needs);
  eval_add(total, 6, reg_t_right);          eval_add(total, 7, needs);
  eval_add(total, 8, correct);              eval_add(total, 9, true);
  eval_add(total, 10, correct_t);           eval_add(total, 11, true);
  if (a.with_histogram && needs) {                   // :528-543: (lo, hi] bins of the relative error; 0 and NaN fall in none
    const float edge[13] = {0.f, (float)(1.0 / 20), (float)(2.0 / 20), (float)(3.0 / 20), (float)(4.0 / 20), (float)(3.0 / 10), (float)(4.0 / 10),
                            (float)(5.0 / 10), (float)(6.0 / 10), (float)(7.0 / 10), (float)(8.0 / 10), (float)(9.0 / 10), (float)(10.0 / 10)};
    int bin = -1;
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (edge[k] < se && se <= edge[k + 1]) bin = k;
    if (1.f < se) bin = 12;
    if (bin >= 0) eval_add(a.tables + CRCT_EVAL_HISTOGRAM, bin, true);
  }
  if (a.cats) {                                      // :465-484: [figure 0 and own][answer kind, and 3 when regressed][category][hit5, hitT, n]
    const int fig = a.cats[3 * q], kind = a.cats[3 * q + 1], qc = a.cats[3 * q + 2];
    if (fig < 1 || fig > 4 || kind < 0 || kind > 2 || qc < 0 || qc > 2) {
      eval_add(a.tables, CRCT_EVAL_ERRORS, true);    // nothing is stored at a bad index
    } else {
      int64_t* bd = a.tables + CRCT_EVAL_BREAKDOWN;
      for (int f = 0; f < 2; ++f) {
        const int row = (f ? fig : 0) * 4;
        for (int r = 0; r < 2; ++r) {
          if (r && !needs) break;
          const int base = ((row + (r ? 3 : kind)) * 3 + qc) * 3;
          eval_add(bd, base, correct); eval_add(bd, base + 1, correct_t); eval_add(bd, base + 2, true);
        }
      }
    }
  }
}

}  // namespace

extern "C" int crct_eval_select(const float* logits, const float* reg_out, const float* reg_err, const float* reg_terr,
                                const int64_t* num_ans, const int64_t* forced_answers, int Q, int64_t N, float* prob0,
                                int64_t* answers, float* sel_out, float* sel_err, float* sel_terr, crct_stream_t stream) {
  CRCT_REQUIRE(logits && reg_out && reg_err && reg_terr && num_ans && answers && sel_out && sel_err && sel_terr,
               "eval_select: null argument");
  CRCT_REQUIRE(Q >= 0 && N >= 0, "eval_select: bad sizes");
  if (Q == 0) return 0;
  crct_launch(eval_select_kernel, dim3(Q), dim3(64), 0, (hipStream_t)stream, logits, reg_out, reg_err, reg_terr, num_ans,
                     forced_answers, Q, (long)N, prob0, answers, sel_out, sel_err, sel_terr);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_eval_score(const CrctEvalScoreArgs* args, crct_stream_t stream) {
  CRCT_REQUIRE(args, "eval_score: null argument struct");
  const CrctEvalScoreArgs& a = *args;
  CRCT_REQUIRE(a.mode == 0 || a.mode == 1, "eval_score: mode %d (0 = candidate rows, 1 = binary answers)", a.mode);
  CRCT_REQUIRE(a.Q >= 0 && a.N >= 0, "eval_score: bad sizes");
  CRCT_REQUIRE(a.logits && a.gt_id && a.needs_reg && a.tolerance && a.answers && a.tables, "eval_score: null argument");
  if (a.mode == 1) {
    CRCT_REQUIRE(a.N == a.Q, "eval_score: binary answers score one row per question, got N %lld for Q %d", (long long)a.N, a.Q);
    CRCT_REQUIRE(a.labels, "eval_score: binary answers need labels");
  } else {
    CRCT_REQUIRE(a.num_ans, "eval_score: candidate rows need num_ans");
    CRCT_REQUIRE(a.reg_out && a.reg_err && a.reg_terr, "eval_score: candidate rows need reg_out, reg_err, reg_terr");
  }
  if (a.Q == 0) return 0;
  crct_launch(eval_score_kernel, dim3(a.Q), dim3(64), 0, (hipStream_t)stream, a);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

// what a score request may ask of a launch: gradient outputs to seed, and a value only where the regressor has a differentiable one
static int score_request(const CrctHeadArgs& a, const CrctScoreGrads* req, bool plotqa, CrctScoreGrads* sg) {
  sg->d_logits = req ? req->d_logits : nullptr;
  sg->d_value = req ? req->d_value : nullptr;
  CRCT_REQUIRE(!sg->d_value || plotqa, "head_loss_scores: d_value: only the PlotQA regressor's value has a gradient (the CE regressor's is a table lookup, without a regressor it is zero)");
  CRCT_REQUIRE(!(sg->d_logits || sg->d_value) || a.d_pooled_t, "head_loss_scores: d_logits / d_value need the gradient outputs (d_pooled_t is NULL: an evaluation launch)");
  return 0;
}

extern "C" int crct_head_loss_scores(const CrctHeadArgs* args, const CrctScoreGrads* scores, crct_stream_t stream) {
  CRCT_REQUIRE(args && args->B > 0 && args->Hb > 0, "head_loss: bad sizes");
  CRCT_REQUIRE(args->scratch, "head_loss: scratch (fp32 [B][8]) is required");
  CrctScoreGrads sg;
  if (const int rc = score_request(*args, scores, true, &sg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  crct_launch(head_rows_kernel<HEAD_PLOTQA>, dim3(args->B), dim3(256), 0, s, *args, args->scratch, HeadValues{}, sg);
  CRCT_CHECK_HIP(hipGetLastError());
  const int nb = ((args->Hb > 256 ? args->Hb : 256) + 31) / 32;
  crct_launch(head_reduce_kernel, dim3(nb), dim3(256), 0, s, *args, (const float*)args->scratch);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_head_loss(const CrctHeadArgs* args, crct_stream_t stream) { return crct_head_loss_scores(args, nullptr, stream); }

extern "C" int crct_head_loss_variant_scores(const CrctHeadVariantArgs* args, const CrctScoreGrads* scores, crct_stream_t stream) {
  CRCT_REQUIRE(args && args->h.B > 0 && args->h.Hb > 0, "head_loss_variant: bad sizes");
  CRCT_REQUIRE(args->h.scratch, "head_loss_variant: scratch (fp32 [B][8]) is required");
  const CrctVariant& v = args->variant;
  CRCT_REQUIRE(v.n_values >= 0 && v.n_values <= CRCT_CE_CLASSES, "head_loss_variant: %d table values (at most %d)", v.n_values, CRCT_CE_CLASSES);
  CrctScoreGrads sg;
  if (const int rc = score_request(args->h, scores, v.regressor == CRCT_REGRESSOR_PLOTQA, &sg)) return rc;
  HeadValues hv = {};
  for (int k = 0; k < v.n_values; ++k) hv.v[k] = v.values[k];
  hv.n = v.n_values;
  hipStream_t s = (hipStream_t)stream;
  const CrctHeadArgs& a = args->h;
  CrctHeadArgs r = a;                     // the reduce pass: bi_seq_relationship gradients + stats (fusion.6 / ce_fusion.6: see below)
  if (v.regressor == CRCT_REGRESSOR_PLOTQA) {
    CRCT_REQUIRE(a.fus_h && a.w_f6 && a.b_f6, "head_loss_variant: the PlotQA regressor needs fus_h, w_f6, b_f6");
    if (args->snap) {
      CRCT_REQUIRE(v.n_values > 0, "head_loss_variant: the DVQA snap needs the value table");
      crct_launch(head_rows_kernel<HEAD_SNAP>, dim3(a.B), dim3(256), 0, s, a, a.scratch, hv, sg);
    } else {
      crct_launch(head_rows_kernel<HEAD_PLOTQA>, dim3(a.B), dim3(256), 0, s, a, a.scratch, hv, sg);
    }
  } else if (v.regressor == CRCT_REGRESSOR_NONE) {
    crct_launch(head_rows_kernel<HEAD_NONE>, dim3(a.B), dim3(256), 0, s, a, a.scratch, hv, sg);
    r.d_w_f6 = nullptr; r.d_b_f6 = nullptr;
  } else if (v.regressor == CRCT_REGRESSOR_CE) {
    CRCT_REQUIRE(v.n_values == CRCT_CE_CLASSES, "head_loss_variant: the CE regressor needs %d table values, got %d", CRCT_CE_CLASSES, v.n_values);
    CRCT_REQUIRE(a.fus_h && a.w_f6 && a.b_f6 && args->ce_scratch, "head_loss_variant: the CE regressor needs fus_h, w_f6, b_f6, ce_scratch");
    crct_launch(head_ce_rows_kernel, dim3(a.B), dim3(256), 0, s, a, a.scratch, args->ce_scratch, hv, sg);
    CRCT_CHECK_HIP(hipGetLastError());
    if (a.d_w_f6) {
      crct_launch(head_ce_wgrad_kernel, dim3(CRCT_CE_CLASSES), dim3(256), 0, s, a, (const float*)args->ce_scratch);
    }
    r.d_w_f6 = nullptr; r.d_b_f6 = nullptr;
  } else {
    CRCT_REQUIRE(false, "head_loss_variant: unknown regressor kind %d", v.regressor);
  }
  CRCT_CHECK_HIP(hipGetLastError());
  const int nb = ((a.Hb > 256 ? a.Hb : 256) + 31) / 32;
  crct_launch(head_reduce_kernel, dim3(nb), dim3(256), 0, s, r, (const float*)a.scratch);
  CRCT_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int crct_head_loss_variant(const CrctHeadVariantArgs* args, crct_stream_t stream) {
  return crct_head_loss_variant_scores(args, nullptr, stream);
}
