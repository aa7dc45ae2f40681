// ita_weights_load.h -- the load-time half of ita_plugin.hip: what one ita_load_weights call builds (Weights) and the
// steps that build it from a blob, in the order the loader runs them.
//
// A part of ita_plugin.hip, its only includer, and not a stand-alone header: ita_plugin.hip defines fail(), HIPCHK,
// DevBuf, with_E, K0P / K0S, launch and the two exact-f32 launch helpers the fold uses (launch_tail, launch_gemm) ahead of the
// #include.
//
// Head counts (header field H): an ITAW0001 blob (int8 attention, int8 FFN) loads with H in {1, 2, 3, 4, 6}; its layers
// then get no stream-kernel images at H > 1 and run on ita_mha_kernel<E, H> + ita_ffn_kernel<E>.  Two refusals stay, both
// ITA_ERR_UNSUPPORTED in check_blob: an ITAW0003 blob (float attention, one head by construction of its kernel) with
// H > 1, and an ITAW0002 blob (int8 attention, float FFN) with H > 1 -- launch_mha would run it, but no fixture of the
// reference pins that graph, so it is not offered.
#pragma once

namespace {

struct Layer {
  const int8_t *wq, *wk, *wv, *wo, *w1, *w2;
  const int32_t *bq, *bk, *bv, *bo, *b1, *b2;
  float ascal[ITA_A_NSCAL], fscal[ITA_F_NSCAL];
  const float *n1w, *n1b, *n2w, *n2b;
  // float32 FFN of an ITAW0002 blob (the attention-only graph), device pointers; the int8 FFN fields are then null
  bool ffn_f32 = false;
  const float *w1f = nullptr, *b1f = nullptr, *w2f = nullptr, *b2f = nullptr;
  DevBuf<float> w1p, w2p;   // E = 128: B-fragment images of W1 / W2 (ita_ffn_f32_frag_image)
  // float32 attention of an ITAW0003 blob (the float graph), device pointers; the int8 attention fields are then null
  bool attn_f32 = false;
  const float *wqf = nullptr, *wkf = nullptr, *wvf = nullptr, *bqf = nullptr, *bkf = nullptr, *bvf = nullptr,
              *wof = nullptr, *bof = nullptr;
  // LDS images of the stream kernels (ita_stream_kernel.h), device copies: whole layer, whole layer with the
  // tokenizer in front (layer 0 of the E = 64 model), attention block only
  DevBuf<char> simg_enc, simg_tok, simg_mha;
  unsigned fast_sites = 0;   // ITA_SITE_* bits: requantisation sites proven equal under single rounding (fast_site_ok)
  // fused requantisation (fused_site): the proven sites among Q, K, V, logits and context (less what ITA_FUSED_SITES turns
  // off), their accumulator bases and K constants in that order, and -- when all five are in, and the layer is fast --
  // second copies of the images with those bases in the Q, K and V biases.  The first copies keep the default base: the
  // long-sequence kernels read simg_mha, the stamped diagnostic instantiations the other two.
  // Entry / bit 5 is fc1 (the fused ReLU form, a proof of its own): with it the whole-layer images carry fc1's base in b1
  // and the FUSED == 2 instantiation runs; without it they keep the default there and FUSED == 1 runs.
  // Entries / bits 6 and 7 are out_proj and fc2 (the fused dequantise form, ita_device.h: dq16_fused): with fc1 and BOTH of
  // them the whole-layer images carry their bases in bo and b2 and FUSED == 3 runs.  The attention-only image keeps the
  // default bo: the int8-I/O form, whose out_proj ends in codes, reads the same image.
  unsigned fused_sites = 0;
  bool fused = false, fused_relu = false, fused_dq = false;
  int fused_c[8] = {ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS};
  float fused_k[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  DevBuf<char> fimg_enc, fimg_tok, fimg_mha;
};

// Everything one ita_load_weights call produces.  Raw pointers point into dblob; every DevBuf is a buffer derived from
// it.  `w = Weights{}` releases the lot and leaves the handle unloaded.
struct Weights {
  bool loaded = false;
  ita_blob_header hdr{};
  std::vector<char> hblob;
  DevBuf<char> dblob;
  std::vector<Layer> layers;
  // float layers (device pointers into dblob)
  const float *tail_b = nullptr, *dec_w = nullptr, *dec_b = nullptr, *fc_w = nullptr, *fc_b = nullptr;
  // derived device buffers
  DevBuf<float> tail_wT;
  DevBuf<char> tok_simg;                   // LDS images of ita_tok_stream_kernel: [u8 frames (conv weights x 1/65280) | f32 frames]
  size_t tok_simg_bytes = 0;               // size of one of the two
  DevBuf<float> wcat[3], bsum[3];
  // split-precision (f16 hi/lo) tail: folded tail+decoder matrix and LSTM weights, pre-scaled
  int kfold = 8192, ldfold = 8192 + 64;    // K and plane row stride of the folded GEMM (see the constants at the top of ita_plugin.hip)
  bool folded = false;
  DevBuf<_Float16> foldf_hi, foldf_lo;     // G0 once more as 16x16x32 MFMA A fragments [N/16][K/32][64][8], for batches of <= 32 frames
  DevBuf<_Float16> fold_hi, fold_lo;       // [512][LDFOLD]: G0 = W_ih0[:, :512] . Wfold, rows in permuted gate order
  DevBuf<float> fold_bias;                 // [512] gate-major: W_ih0[:, :512] . dec(tail(0)) + b_ih0 + b_hh0
  float fold_inv_scale = 1.0f;
  DevBuf<_Float16> lw_hi[3], lw_lo[3];     // [512][K0S | 256 | 256]
  float lw_inv_scale[3] = {1.0f, 1.0f, 1.0f};
};

template <typename T>
const T* dptr(const Weights& w, const char* name, bool required, bool* ok) {
  const ita_blob_entry* e = ita_blob_find(w.hblob.data(), w.hblob.size(), name);
  if (!e) {
    if (required) *ok = false;
    return nullptr;
  }
  return (const T*)(w.dblob + e->offset);
}
template <typename T>
const T* hptr(const Weights& w, const char* name) {
  const ita_blob_entry* e = ita_blob_find(w.hblob.data(), w.hblob.size(), name);
  return e ? (const T*)(w.hblob.data() + e->offset) : nullptr;
}

// ---- IEEE binary16 <-> binary32 on the host (also used by the host-buffer drop-in symbols)
float half_to_float(uint16_t hbits) {
  const uint32_t sign = (uint32_t)(hbits & 0x8000u) << 16;
  uint32_t exp = (hbits >> 10) & 0x1fu, man = hbits & 0x3ffu, out;
  if (exp == 0) {
    if (man == 0) out = sign;
    else {
      exp = 127 - 15 + 1;
      while (!(man & 0x400u)) { man <<= 1; --exp; }
      out = sign | (exp << 23) | ((man & 0x3ffu) << 13);
    }
  } else if (exp == 31) out = sign | 0x7f800000u | (man << 13);
  else out = sign | ((exp + 127 - 15) << 23) | (man << 13);
  float f;
  memcpy(&f, &out, 4);
  return f;
}
uint16_t float_to_half(float f) {   // round to nearest even
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  const uint32_t absx = x & 0x7fffffffu;
  if (absx >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (absx > 0x7f800000u ? 0x200u : 0));
  if (absx >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);            // overflow -> inf
  if (absx < 0x33000001u) return sign;                                    // underflow -> 0
  int exp = (int)(absx >> 23) - 127 + 15;
  uint32_t man = (absx & 0x7fffffu) | 0x800000u;
  int shift = 13;
  if (exp <= 0) { shift += 1 - exp; exp = 0; }
  uint32_t hm = man >> shift;
  const uint32_t rem = man & ((1u << shift) - 1), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (hm & 1))) ++hm;
  uint32_t outv = exp > 0 ? (((uint32_t)exp << 10) + (hm - 0x400u)) : hm;   // mantissa carry bumps the exponent
  return (uint16_t)(sign | outv);
}

// ---- split precision: a weight tensor travels as two f16 planes of w * 2^e, e chosen so that max|w| * 2^e lies in
// [512, 1024), which keeps the lo halves normal in f16
int split_scale_exp(float max_abs) {
  if (!(max_abs > 0.0f)) return 0;
  int ex;
  (void)frexpf(max_abs, &ex);   // max_abs = m * 2^ex, m in [0.5, 1)
  return 10 - ex;
}
void split_half(float v, uint16_t* hi, uint16_t* lo) {   // v already scaled: hi = half(v), lo = half(v - hi)
  *hi = float_to_half(v);
  *lo = float_to_half(v - half_to_float(*hi));
}
float max_abs_of(const float* w, size_t n) {
  float mx = 0.0f;
  for (size_t i = 0; i < n; ++i) mx = fabsf(w[i]) > mx ? fabsf(w[i]) : mx;
  return mx;
}
int split_upload(const std::vector<float>& w, DevBuf<_Float16>& d_hi, DevBuf<_Float16>& d_lo, float* inv_scale) {
  const int e = split_scale_exp(max_abs_of(w.data(), w.size()));
  const float sc = ldexpf(1.0f, e);
  *inv_scale = ldexpf(1.0f, -e);
  std::vector<uint16_t> hi(w.size()), lo(w.size());
  for (size_t i = 0; i < w.size(); ++i) split_half(w[i] * sc, &hi[i], &lo[i]);
  HIPCHK(d_hi.upload((const _Float16*)hi.data(), hi.size()));
  HIPCHK(d_lo.upload((const _Float16*)lo.data(), lo.size()));
  return ITA_OK;
}

// ---- stream kernels (ita_stream_kernel.h): the LDS image a workgroup copies verbatim at start-up.
// Natural-k matrices (Wq, Wk, Wv, W1) are chunk-major [k/16][row][16].  The block output projections (Wo, fc2)
// consume activations that were packed four 16-feature tiles at a time straight from MFMA accumulators:
// fragment ks of lane (token, kq) holds, at byte 4j+i, feature 16(4ks+j) + 4kq + i -- so chunk 4ks+kq of their
// image holds those input features, and image row 16et + rho is output channel (E/4)(rho>>2) + 4et + (rho&3),
// which hands lane (token, kq) its own channels (E/4)kq + 4et + i.
struct StreamHostParams {
  const int8_t *wq, *wk, *wv, *wo, *w1, *w2;
  const int32_t *bq, *bk, *bv, *bo, *b1, *b2;
  const float *n1w, *n1b, *n2w, *n2b, *tlw, *tlb, *conv_w, *conv_b;
};

// the tokenizers' tap table, int32 [52]: offset ky * 96 + kx of tap t in a 9 x 96 pixel window, 0 for the pad taps 49..51
void fill_tok_taps(char* at) {
  int32_t* tap = (int32_t*)at;
  for (int t = 0; t < 52; ++t) tap[t] = t < 49 ? (t / 7) * 96 + (t % 7) : 0;
}

// The integer conv tables of the u8 tokenizer (ita_tokenizer_kernel.h: ItaTokTab; definition: oracle/ita_oracle.c
// ita_oracle_tok_quant_weights / ita_oracle_tokenizer_u8): per channel 23-bit fixed-point weights Wq = rne(w * 2^e), e = 22 -
// exponent(max |w|), split into balanced bytes w0, w1 and the remainder w2, laid out as int8 MFMA A fragments.
template <int E>
void build_tok_tab(const float* conv_w, const float* conv_b, char* tab) {
  using T = ItaTokTab<E>;
  int32_t* ti = (int32_t*)(tab + T::TI);
  float* ts = (float*)(tab + T::TS);
  std::vector<int8_t> dig((size_t)E * 49 * 3);
  for (int c = 0; c < E; ++c) {
    float mx = 0.0f;
    for (int k = 0; k < 49; ++k) mx = fmaxf(mx, fabsf(conv_w[(size_t)c * 49 + k]));
    int e = 0;
    if (mx > 0.0f) {
      int ex;
      (void)frexpf(mx, &ex);
      e = 22 - ex;
    }
    long long s0 = 0, s1 = 0, s2 = 0;
    for (int k = 0; k < 49; ++k) {
      const int32_t W = (int32_t)rintf(ldexpf(conv_w[(size_t)c * 49 + k], e));
      const int32_t w0 = ((W + 128) & 255) - 128, W1r = (W - w0) >> 8;
      const int32_t w1 = ((W1r + 128) & 255) - 128, w2 = (W1r - w1) >> 8;
      dig[((size_t)c * 49 + k) * 3 + 0] = (int8_t)w0; dig[((size_t)c * 49 + k) * 3 + 1] = (int8_t)w1; dig[((size_t)c * 49 + k) * 3 + 2] = (int8_t)w2;
      s0 += w0; s1 += w1; s2 += w2;
    }
    // the kernel feeds a ^ 0x80 = a - 128: S0 = S0' + 128 sum w0, S1 = S1' + 128 (sum w1 + sum w0), ... (L = S0 + 256 S1, H = S2 + 256 S3)
    ti[c] = (int32_t)(128 * s0 + 256 * 128 * (s1 + s0));
    ti[E + c] = (int32_t)(128 * (s2 + s1) + 256 * 128 * s2);
    const float sc = ldexpf(1.0f, -e) / 65280.0f;
    ts[c] = sc; ts[E + c] = 65536.0f * sc; ts[2 * E + c] = conv_b[c];
  }
  for (int ct = 0; ct < T::NCT; ++ct)
    for (int j = 0; j < 3; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        const int rho = lane & 15, kq = lane >> 4, ch = (E / 4) * (rho >> 2) + 4 * ct + (rho & 3);
        for (int b = 0; b < 16; ++b) {
          const int t = 4 * b + kq;        // slot b of k-group kq <-> tap 4 b + kq (the lane that blends it); taps >= 49: zero
          tab[T::TW + ((ct * 3 + j) * 64 + lane) * 16 + b] = t < 49 ? (char)dig[((size_t)ch * 49 + t) * 3 + j] : 0;
        }
      }
}

// cb: the accumulator bases of the Q, K, V, fc1, out_proj and fc2 sites (fused form: Layer::fused_c[0, 1, 2, 5, 6, 7]), or
// null: ITA_ACC_BIAS
template <int E, bool FFN, bool TOK>
int build_stream_image(const StreamHostParams& p, DevBuf<char>& out, const int* cb = nullptr) {
  using L = ItaStreamLds<E, FFN, TOK>;
  constexpr int P = 192, F = 256;
  std::vector<char> im(L::GIMAGE, 0);   // (E = 128 with FFN: fc1 / fc2 weights lie behind the LDS part)
  auto natural = [&](int off, const int8_t* w, int rows, int kb) {
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < kb; ++k) im[off + (((k >> 4) * rows + r) << 4) + (k & 15)] = (char)w[(size_t)r * kb + k];
  };
  auto fragment = [&](int off, const int8_t* w, int nks, int kb) {   // w: [E][kb], kb = 64 * nks
    for (int ks = 0; ks < nks; ++ks)
      for (int kq = 0; kq < 4; ++kq)
        for (int et = 0; et < E / 16; ++et)
          for (int rho = 0; rho < 16; ++rho) {
            const int ch = (E / 4) * (rho >> 2) + 4 * et + (rho & 3);
            for (int j = 0; j < 4; ++j)
              for (int i = 0; i < 4; ++i)
                im[off + (((4 * ks + kq) * E + et * 16 + rho) << 4) + 4 * j + i] =
                    (char)w[(size_t)ch * kb + (4 * ks + j) * 16 + 4 * kq + i];
          }
  };
  natural(L::WQ, p.wq, P, E); natural(L::WK, p.wk, P, E); natural(L::WV, p.wv, P, E);
  fragment(L::WO, p.wo, 3, P);
  int32_t* bias = (int32_t*)(im.data() + L::BIAS);
  memcpy(bias, p.bq, P * 4); memcpy(bias + P, p.bk, P * 4); memcpy(bias + 2 * P, p.bv, P * 4);
  memcpy(bias + 3 * P, p.bo, E * 4);
  float* ln = (float*)(im.data() + L::LNP);
  if (p.n1w && p.n1b) { memcpy(ln, p.n1w, E * 4); memcpy(ln + E, p.n1b, E * 4); }
  auto bias_accumulators = [&]() {   // accumulators start at ITA_ACC_BIAS + bias (ita_device.h: scale_clamp_b)
    for (int i = 0; i < L::NBIAS; ++i) {
      int base = ITA_ACC_BIAS;
      if (cb && i < 3 * P) base = cb[i / P];
      else if (cb && FFN && i < 3 * P + E) base = cb[6];
      else if (cb && FFN && i < 3 * P + E + F) base = cb[5];
      else if (cb && FFN) base = cb[7];
      bias[i] = (int32_t)((uint32_t)bias[i] + (uint32_t)base);
    }
  };
  if constexpr (FFN) {
    natural(L::W12G ? L::GW1 : L::W1, p.w1, F, E);
    fragment(L::W12G ? L::GW2 : L::W2, p.w2, 4, F);
    memcpy(bias + 3 * P + E, p.b1, F * 4); memcpy(bias + 3 * P + E + F, p.b2, E * 4);
    memcpy(ln + 2 * E, p.n2w, E * 4); memcpy(ln + 3 * E, p.n2b, E * 4);
  }
  if constexpr (TOK) {
    memcpy(ln + 4 * E, p.tlw, E * 4); memcpy(ln + 5 * E, p.tlb, E * 4);
    build_tok_tab<E>(p.conv_w, p.conv_b, im.data() + L::CW);
    fill_tok_taps(im.data() + L::TAP);
  }
  bias_accumulators();
  {
    int32_t* vb4 = (int32_t*)(im.data() + L::VB4);
    for (int d = 0; d < P; ++d)
      for (int i = 0; i < 4; ++i) vb4[4 * d + i] = bias[2 * P + d];
  }
  HIPCHK(out.upload(im.data(), im.size()));
  return ITA_OK;
}

// The stream kernels read an int32 accumulator as the float 1.5 * 2^23 + sum, which is exact while |sum| < 2^22.
// Worst case of a Linear row: sum_k |w| * 128 + |bias| (inputs are int8 codes).  QK^T (192 * 128 * 128) and A.V
// (<= 255 * 128) are inside the range by construction.  A blob outside it runs on the block kernels instead.
bool stream_range_ok(const StreamHostParams& p, int E, bool ffn, const float* ascal, const float* fscal) {
  // ... and the requantised value travels as a 16-bit integer between the rounding and the u8 saturation
  // (ita_device.h: rq_pack16_v3), so |acc * mult| + 128 has to stay below 2^15 as well: same worst case times the multiplier.
  auto rows_ok = [](const int8_t* w, const int32_t* b, int rows, int k, float mult) {
    if (!(mult > 0.0f)) return false;
    for (int r = 0; r < rows; ++r) {
      long long sum = 0;
      for (int i = 0; i < k; ++i) sum += w[(size_t)r * k + i] < 0 ? -(long long)w[(size_t)r * k + i] : w[(size_t)r * k + i];
      const long long bb = b[r] < 0 ? -(long long)b[r] : b[r];
      if (sum * 128 + bb >= (1ll << 22)) return false;
      if ((double)(sum * 128 + bb) * (double)mult >= 32000.0) return false;
    }
    return true;
  };
  if (!(ascal[ITA_A_ML] > 0.0f) || 192.0 * 128 * 128 * (double)ascal[ITA_A_ML] >= 32000.0) return false;   // Q K^T
  // A V: the integer softmax's probabilities sum to at most 255 per row (each is floor(num * 255 / sum(num))), so |sum p v| <= 255 * 128
  if (!(ascal[ITA_A_MC] > 0.0f) || 255.0 * 128 * (double)ascal[ITA_A_MC] >= 32000.0) return false;
  return rows_ok(p.wq, p.bq, 192, E, ascal[ITA_A_MQ]) && rows_ok(p.wk, p.bk, 192, E, ascal[ITA_A_MK]) &&
         rows_ok(p.wv, p.bv, 192, E, ascal[ITA_A_MV]) && rows_ok(p.wo, p.bo, E, 192, ascal[ITA_A_MO]) &&
         (!ffn || (rows_ok(p.w1, p.b1, 256, E, fscal[ITA_F_M1]) && rows_ok(p.w2, p.b2, E, 256, fscal[ITA_F_M2])));
}

// Single-rounding permission of one requantisation site.  The reference computes rne(fl(acc * m)) -- two roundings; the
// fast form of the stream kernels computes fl(acc * m + magic) in one fused multiply-add -- one rounding.  They can differ
// only for an accumulator value whose exact product lies within half an ulp of a rounding tie without being one.  The set of
// accumulator values that matter is small (|acc * m| below the clamp range: a few hundred thousand integers), so it is
// simply enumerated, on the host, in the arithmetic the GPU instructions perform (IEEE f32 multiply, add and fma; this file
// is compiled with -ffp-contract=off): a site is fast only if no value differs after the clamp.
bool fast_site_ok(float m) {
  if (!(m > 0.0f) || !(m < 1.0f)) return false;
  const double lim = 130.0 / (double)m;
  if (lim > 4.0e6) return false;   // outside the biased-float accumulator range: not a stream-kernel blob anyway
  const long long A = (long long)lim + 2;
  auto code = [](float t) {        // low 16 bits of the pattern = r + 128 (two's complement), then the u8 saturation
    unsigned u;
    memcpy(&u, &t, 4);
    const int v = (int)(int16_t)(u & 0xffffu);
    return v < 0 ? 0 : v > 255 ? 255 : v;
  };
  for (long long a = -A; a <= A; ++a) {
    const float x = (float)a;
    const float y = x * m;
    if (code(y + ITA_MAGIC128_F) != code(fmaf(x, m, ITA_MAGIC128_F))) return false;
  }
  return true;
}
unsigned fast_sites_of(const float* ascal) {
  unsigned mask = 0;
  const int idx[6] = {ITA_A_MQ, ITA_A_MK, ITA_A_MV, ITA_A_ML, ITA_A_MC, ITA_A_MO};
  for (int i = 0; i < 6; ++i)
    if (fast_site_ok(ascal[idx[i]])) mask |= 1u << i;   // bit order = ITA_SITE_Q, _K, _V, _L, _C, _O
  return mask;
}

// Fused requantisation of one site: the accumulator starts at an integer C near 1.5 * 2^23 instead of at it, its bit pattern
// is still the float C + sum, and ONE fma(C + sum, m, K) with K = magic - k, k = round(C m), yields rne(sum m + magic + eps),
// eps = C m - k: no subtraction of the base.  The search takes the C within +-dmax of ITA_ACC_BIAS whose C m lies closest to
// an integer (exact integer arithmetic on m's mantissa), and for the best few enumerates every accumulator value of the
// clamp range -- the range fast_site_ok walks -- in the arithmetic of v_pk_fma_f32 (IEEE fmaf; this file is compiled with
// contraction off): a C is accepted when the clamped code equals that of the reference's two roundings for every value.
// magic: ITA_MAGIC128_F (codes travel as r + 128, u8 saturation), ITA_MAGIC32K_F (logits: r + 32768, clamped by the
// integer softmax, which reads nothing of a logit but its clamped value: ita_softmax_packed16) or ITA_MAGIC_F (fc1's fused
// ReLU form: r itself travels, min with 127 and the u8 saturation clamp it to [0, 127]; dq, the dequantise sites out_proj and
// fc2: r = t - 1.5 * 2^23 as a float, exact, clamped to [-128, 127] by v_med3_f32 -- nothing travels in 16 bits).
constexpr int ITA_FUSED_DMAX = 1 << 18, ITA_FUSED_TRIES = 8;
// the enumeration for one given C: true when the fused form equals the reference on the whole clamp range; *K is set whenever
// K is an exact float in [2^23, 2^24)
bool fused_site_check(float m, float magic, int C, float* K, bool dq = false) {
  if (!(m > 0.0f) || !(m < 1.0f)) return false;
  const double lim = 130.0 / (double)m;
  if (lim > 4.0e6) return false;
  const long long dC = (long long)C - (long long)ITA_ACC_BIAS;
  if (dC < -(1ll << 22) || dC >= (1ll << 22)) return false;
  const long long A = (long long)lim + 2;
  if (A + (dC < 0 ? -dC : dC) >= (1ll << 22)) return false;   // C + a must stay a float with ulp 1: [2^23, 2^24)
  // (the pattern 0x4B000000 + t is the float 2^23 + t; a 24-bit integer times a 24-bit mantissa is exact in double)
  const double cval = (double)((long long)C - 0x4B000000ll) + 8388608.0;
  const double k = nearbyint(cval * (double)m);
  const double kd = (double)magic - k;
  if (!(kd >= 8388608.0) || !(kd < 16777216.0)) return false;
  const float Kf = (float)kd;                                 // an integer below 2^24: exact
  *K = Kf;
  const bool l16 = magic == ITA_MAGIC32K_F, relu = magic == ITA_MAGIC_F;
  if (dq && !relu) return false;   // the dequantise form is defined against K = 1.5 * 2^23 - round(C m) only
  auto code = [l16, relu, dq](float t) {
    if (dq) {    // t is an integer of [2^23, 2^24): the subtraction is exact, then the float clamp
      const float r = t - ITA_MAGIC_F;
      return (int)(r < -128.0f ? -128.0f : r > 127.0f ? 127.0f : r);
    }
    unsigned u;
    memcpy(&u, &t, 4);
    if (relu) {   // low 16 bits = r, signed
      const int v = (int)(int16_t)(u & 0xffffu);
      return v < 0 ? 0 : v > 127 ? 127 : v;
    }
    if (l16) {   // low 16 bits = r + 32768 (unsigned); the softmax clamps r to [-128, 127]
      const int v = (int)(u & 0xffffu) - 32768;
      return v < -128 ? -128 : v > 127 ? 127 : v;
    }
    const int v = (int)(int16_t)(u & 0xffffu);   // r + 128, then the u8 saturation
    return v < 0 ? 0 : v > 255 ? 255 : v;
  };
  for (long long a = -A; a <= A; ++a) {
    const float y = (float)a * m;
    uint32_t bits = (uint32_t)((long long)C + a);
    float f;
    memcpy(&f, &bits, 4);
    if (code(y + magic) != code(fmaf(f, m, Kf))) return false;
  }
  return true;
}
// the search: *C, *K of the first accepted candidate
bool fused_site(float m, float magic, int dmax, int* C, float* K, bool dq = false) {
  if (!(m > 0.0f) || !(m < 1.0f) || 130.0 / (double)m > 4.0e6 || dmax < 0) return false;
  if (dmax > ITA_FUSED_DMAX) dmax = ITA_FUSED_DMAX;
  uint32_t mb;
  memcpy(&mb, &m, 4);
  const int ex = (int)(mb >> 23);
  if (ex == 0) return false;                                  // (a denormal multiplier is below the range bound anyway)
  const uint64_t M = (mb & 0x7fffffu) | 0x800000u;            // m = M * 2^-s
  const int s = 150 - ex;                                     // m < 1: s >= 24; 130 / m <= 4e6: s <= 39
  if (s < 24 || s > 39) return false;
  const uint64_t one = 1ull << s, mask = one - 1;
  struct Cand { uint64_t d; int C; };
  Cand best[ITA_FUSED_TRIES];
  int nb = 0;
  const long long c0 = (long long)ITA_ACC_BIAS - 0x4B000000ll + 8388608ll;   // the float value of the default base
  for (int d = -dmax; d <= dmax; ++d) {
    const uint64_t fr = ((uint64_t)(c0 + d) * M) & mask;      // (C M) mod 2^s: below 2^24 * 2^24, exact
    const uint64_t dist = fr < one - fr ? fr : one - fr;
    if (nb == ITA_FUSED_TRIES && dist >= best[nb - 1].d) continue;
    int j = nb < ITA_FUSED_TRIES ? nb++ : nb - 1;
    while (j > 0 && best[j - 1].d > dist) { best[j] = best[j - 1]; --j; }
    best[j] = Cand{dist, (int)((long long)ITA_ACC_BIAS + d)};
  }
  for (int i = 0; i < nb; ++i)
    if (fused_site_check(m, magic, best[i].C, K, dq)) { *C = best[i].C; return true; }
  return false;
}

// The fused sites of a layer whose accumulators stream_range_ok admitted: Q, K, V (bases in the image's biases: the base
// may move only as far as the worst row sum leaves room below 2^22), logits (|sum| <= 192 * 128 * 128) and context
// (<= 255 * 128); fc1, and the two dequantise sites out_proj and fc2, of a whole layer (bases in b1, bo, b2).
// ITA_FUSED_SITES (diagnostic, read at load time) is ANDed onto the proven mask: it can only turn sites off.
void prove_fused(Layer& L, const StreamHostParams& p, int E, bool ffn) {
  auto room = [](const int8_t* w, const int32_t* b, int rows, int k) {
    long long worst = 0;
    for (int r = 0; r < rows; ++r) {
      long long sum = 0;
      for (int i = 0; i < k; ++i) sum += w[(size_t)r * k + i] < 0 ? -(long long)w[(size_t)r * k + i] : w[(size_t)r * k + i];
      sum = sum * 128 + (b[r] < 0 ? -(long long)b[r] : b[r]);
      worst = sum > worst ? sum : worst;
    }
    return (int)((1ll << 22) - 1 - worst);   // (stream_range_ok: worst < 2^22)
  };
  const int idx[5] = {ITA_A_MQ, ITA_A_MK, ITA_A_MV, ITA_A_ML, ITA_A_MC};
  const int dmax[5] = {room(p.wq, p.bq, 192, E), room(p.wk, p.bk, 192, E), room(p.wv, p.bv, 192, E),
                       (1 << 22) - 1 - 192 * 128 * 128, (1 << 22) - 1 - 255 * 128};
  unsigned proven = 0;
  for (int i = 0; i < 5; ++i)
    if (fused_site(L.ascal[idx[i]], i == 3 ? ITA_MAGIC32K_F : ITA_MAGIC128_F, dmax[i], &L.fused_c[i], &L.fused_k[i])) proven |= 1u << i;
  unsigned mask = ITA_SITES_FUSED | ITA_SITE_FC1 | ITA_SITES_DQ;
  if (const char* e = getenv("ITA_FUSED_SITES")) mask = (unsigned)strtoul(e, nullptr, 0);
  if (ffn && fused_site(L.fscal[ITA_F_M1], ITA_MAGIC_F, room(p.w1, p.b1, 256, E), &L.fused_c[5], &L.fused_k[5])) proven |= ITA_SITE_FC1;
  if (ffn && fused_site(L.ascal[ITA_A_MO], ITA_MAGIC_F, room(p.wo, p.bo, E, 192), &L.fused_c[6], &L.fused_k[6], true)) proven |= ITA_SITE_DQ_O;
  if (ffn && fused_site(L.fscal[ITA_F_M2], ITA_MAGIC_F, room(p.w2, p.b2, E, 256), &L.fused_c[7], &L.fused_k[7], true)) proven |= ITA_SITE_DQ_FC2;
  mask &= proven;
  L.fused_sites = mask;
  L.fused = (mask & ITA_SITES_FUSED) == ITA_SITES_FUSED && L.fast_sites == ITA_SITES_ALL;
  L.fused_relu = L.fused && (mask & ITA_SITE_FC1);
  L.fused_dq = L.fused_relu && (mask & ITA_SITES_DQ) == ITA_SITES_DQ;
  if (!L.fused_relu) L.fused_c[5] = ITA_ACC_BIAS;   // the images keep fc1's default base
  if (!L.fused_dq) L.fused_c[6] = L.fused_c[7] = ITA_ACC_BIAS;   // ... and out_proj's and fc2's
}

// ---- the steps of ita_load_weights, in the order the loader runs them; each returns an ITA_* code, and the loader
// resets the Weights on any failure, so none of them cleans up after itself
struct BlobKinds { int ffn, attn; };   // ita_blob_ffn_kind / ita_blob_attn_kind: 0 = int8, 1 = float32

#define NM(fmt) (snprintf(nm, sizeof nm, fmt, i), nm)   // tensor name of layer i, in the local buffer nm

// step 1: the header and the tensor table, before anything of the handle is touched
int check_blob(const void* blob, size_t nbytes, ita_blob_header* hdr_out, BlobKinds* kinds) {
  const int ffn_kind = nbytes < sizeof(ita_blob_header) ? -1 : ita_blob_ffn_kind(blob, nbytes);
  const int attn_kind = nbytes < sizeof(ita_blob_header) ? -1 : ita_blob_attn_kind(blob, nbytes);
  if (ffn_kind < 0 || attn_kind < 0) return fail(ITA_ERR_BAD_BLOB, "not an ITAW0001 / ITAW0002 / ITAW0003 blob");
  ita_blob_header hdr;
  memcpy(&hdr, blob, sizeof hdr);
  if (hdr.n_tensors < 0 || sizeof(hdr) + (size_t)hdr.n_tensors * sizeof(ita_blob_entry) > nbytes)
    return fail(ITA_ERR_BAD_BLOB, "tensor table exceeds the blob");
  const bool heads_ok = hdr.H == 1 || hdr.H == 2 || hdr.H == 3 || hdr.H == 4 || hdr.H == 6;
  if ((hdr.E != 64 && hdr.E != 128) || hdr.S != 128 || hdr.P != 192 || hdr.F != 256 || !heads_ok ||
      hdr.num_layers < 1 || hdr.num_layers > 16)
    return fail(ITA_ERR_UNSUPPORTED, "kernels are built for E in {64,128}, S=128, P=192, F=256, H in {1,2,3,4,6}");
  // heads run on the int8 block attention kernel of an all-int8 blob only: the float attention kernel (ITAW0003) has
  // one head, and the attention-only graph (ITAW0002) is not tested with more
  if (hdr.H != 1 && (attn_kind != 0 || ffn_kind != 0))
    return fail(ITA_ERR_UNSUPPORTED, "H > 1 needs an ITAW0001 blob (int8 attention and int8 FFN)");
  // the float graph (ITAW0003) runs at E = 64 with its fusion tail, and at E = 128 without one (ITA_upsample_shuffle)
  if (attn_kind == 1 && hdr.E != 64 && hdr.has_tail)
    return fail(ITA_ERR_UNSUPPORTED, "the float32 graph's fusion tail (ITAW0003) is built for E = 64; at E = 128 it runs without one");
  if (attn_kind == 0 && ffn_kind == 1 && hdr.E != 64) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN (ITAW0002) is built for E = 64");
  const ita_blob_entry* e = (const ita_blob_entry*)((const char*)blob + sizeof(hdr));
  for (int i = 0; i < hdr.n_tensors; ++i)
    if (e[i].offset < 0 || e[i].nbytes < 0 || (size_t)e[i].offset + (size_t)e[i].nbytes > nbytes || (e[i].offset & 15))
      return fail(ITA_ERR_BAD_BLOB, "tensor out of bounds or misaligned");
  char bad[32];
  const int v = ita_blob_validate(blob, nbytes, bad);
  if (v) return fail(ITA_ERR_BAD_BLOB, std::string(v == -2 ? "required tensor missing: " : v == -3 ? "tensor has the wrong dtype or size: " : "malformed blob ") + bad);
  *hdr_out = hdr;
  *kinds = BlobKinds{ffn_kind, attn_kind};
  return ITA_OK;
}

// step 2: the layers' and the float tail's pointers into the uploaded blob (w.hdr, w.hblob and w.dblob are in place)
int bind_layers(Weights& w, BlobKinds kinds) {
  const ita_blob_header& hdr = w.hdr;
  bool ok = true;
  w.layers = std::vector<Layer>(hdr.num_layers);
  char nm[40];
  auto expect = [&](const char* name, size_t bytes) {
    const ita_blob_entry* e = ita_blob_find(w.hblob.data(), w.hblob.size(), name);
    if (e && (size_t)e->nbytes != bytes) ok = false;
  };
  const size_t E = hdr.E, P = hdr.P, F = hdr.F;
  for (int i = 0; i < hdr.num_layers; ++i) {
    Layer& L = w.layers[i];
    if (kinds.attn == 1) {   // float32 attention (sizes checked by ita_blob_validate)
      L.attn_f32 = true;
      L.wqf = dptr<float>(w, NM("attn%d.wqf"), true, &ok); L.wkf = dptr<float>(w, NM("attn%d.wkf"), true, &ok);
      L.wvf = dptr<float>(w, NM("attn%d.wvf"), true, &ok); L.bqf = dptr<float>(w, NM("attn%d.bqf"), true, &ok);
      L.bkf = dptr<float>(w, NM("attn%d.bkf"), true, &ok); L.bvf = dptr<float>(w, NM("attn%d.bvf"), true, &ok);
      L.wof = dptr<float>(w, NM("attn%d.wof"), true, &ok); L.bof = dptr<float>(w, NM("attn%d.bof"), true, &ok);
    } else {
      expect(NM("attn%d.wq"), P * E); expect(NM("attn%d.wo"), E * P); expect(NM("attn%d.bq"), P * 4);
      expect(NM("attn%d.bo"), E * 4); expect(NM("attn%d.scal"), ITA_A_NSCAL * 4);
      L.wq = dptr<int8_t>(w, NM("attn%d.wq"), true, &ok); L.wk = dptr<int8_t>(w, NM("attn%d.wk"), true, &ok);
      L.wv = dptr<int8_t>(w, NM("attn%d.wv"), true, &ok); L.wo = dptr<int8_t>(w, NM("attn%d.wo"), true, &ok);
      L.bq = dptr<int32_t>(w, NM("attn%d.bq"), true, &ok); L.bk = dptr<int32_t>(w, NM("attn%d.bk"), true, &ok);
      L.bv = dptr<int32_t>(w, NM("attn%d.bv"), true, &ok); L.bo = dptr<int32_t>(w, NM("attn%d.bo"), true, &ok);
      const float* as = hptr<float>(w, NM("attn%d.scal"));
      if (!as) { ok = false; break; }
      memcpy(L.ascal, as, sizeof L.ascal);
    }
    if (kinds.ffn == 1) {   // float32 FFN (sizes checked by ita_blob_validate)
      L.ffn_f32 = true;
      L.w1f = dptr<float>(w, NM("ffn%d.w1f"), true, &ok); L.b1f = dptr<float>(w, NM("ffn%d.b1f"), true, &ok);
      L.w2f = dptr<float>(w, NM("ffn%d.w2f"), true, &ok); L.b2f = dptr<float>(w, NM("ffn%d.b2f"), true, &ok);
      const float *w1 = hptr<float>(w, NM("ffn%d.w1f")), *w2 = hptr<float>(w, NM("ffn%d.w2f"));
      if (E == 128 && w1 && w2) {   // ita_ffn_f32_kernel<128> streams W1 / W2 as B-fragment images
        std::vector<float> img(F * E);
        ita_ffn_f32_frag_image(w1, (int)F, (int)E, img.data());
        const bool up1 = L.w1p.upload(img.data(), img.size()) == hipSuccess;
        ita_ffn_f32_frag_image(w2, (int)E, (int)F, img.data());
        if (!up1 || L.w2p.upload(img.data(), img.size()) != hipSuccess)
          return fail(ITA_ERR_HIP, "uploading the float32 FFN fragment images failed");
      }
    } else {
      expect(NM("ffn%d.w1"), F * E); expect(NM("ffn%d.w2"), E * F); expect(NM("ffn%d.scal"), ITA_F_NSCAL * 4);
      L.w1 = dptr<int8_t>(w, NM("ffn%d.w1"), true, &ok); L.w2 = dptr<int8_t>(w, NM("ffn%d.w2"), true, &ok);
      L.b1 = dptr<int32_t>(w, NM("ffn%d.b1"), true, &ok); L.b2 = dptr<int32_t>(w, NM("ffn%d.b2"), true, &ok);
      const float* fs = hptr<float>(w, NM("ffn%d.scal"));
      if (!fs) { ok = false; break; }
      memcpy(L.fscal, fs, sizeof L.fscal);
    }
    L.n1w = dptr<float>(w, NM("norm1_%d.w"), false, &ok); L.n1b = dptr<float>(w, NM("norm1_%d.b"), false, &ok);
    L.n2w = dptr<float>(w, NM("norm2_%d.w"), false, &ok); L.n2b = dptr<float>(w, NM("norm2_%d.b"), false, &ok);
  }
  if (!ok) return fail(ITA_ERR_BAD_BLOB, "a required block tensor is missing or mis-sized");
  w.tail_b = dptr<float>(w, "tail.conv_b", false, &ok);
  w.dec_w = dptr<float>(w, "dec.w", false, &ok); w.dec_b = dptr<float>(w, "dec.b", false, &ok);
  w.fc_w = dptr<float>(w, "fc.w", false, &ok); w.fc_b = dptr<float>(w, "fc.b", false, &ok);
  return ITA_OK;
}

// step 3: the LDS images of the stream kernels, for every int8-attention layer whose accumulators stay in range
int build_stream_images(Weights& w) {
  const ita_blob_header& hdr = w.hdr;
  char nm[40];
  for (int i = 0; i < hdr.num_layers; ++i) {
    Layer& L = w.layers[i];
    if (L.attn_f32) continue;   // no int8 attention: no stream images (ita_attn_f32_kernel + ita_ffn_f32_kernel)
    if (hdr.H != 1) continue;   // the stream kernels have one head: a multi-head layer runs on the block kernels
    StreamHostParams sp{};
    sp.wq = hptr<int8_t>(w, NM("attn%d.wq")); sp.wk = hptr<int8_t>(w, NM("attn%d.wk")); sp.wv = hptr<int8_t>(w, NM("attn%d.wv"));
    sp.wo = hptr<int8_t>(w, NM("attn%d.wo")); sp.w1 = hptr<int8_t>(w, NM("ffn%d.w1")); sp.w2 = hptr<int8_t>(w, NM("ffn%d.w2"));
    sp.bq = hptr<int32_t>(w, NM("attn%d.bq")); sp.bk = hptr<int32_t>(w, NM("attn%d.bk")); sp.bv = hptr<int32_t>(w, NM("attn%d.bv"));
    sp.bo = hptr<int32_t>(w, NM("attn%d.bo")); sp.b1 = hptr<int32_t>(w, NM("ffn%d.b1")); sp.b2 = hptr<int32_t>(w, NM("ffn%d.b2"));
    sp.n1w = hptr<float>(w, NM("norm1_%d.w")); sp.n1b = hptr<float>(w, NM("norm1_%d.b"));
    sp.n2w = hptr<float>(w, NM("norm2_%d.w")); sp.n2b = hptr<float>(w, NM("norm2_%d.b"));
    sp.tlw = hptr<float>(w, "tok.ln_w"); sp.tlb = hptr<float>(w, "tok.ln_b");
    sp.conv_w = hptr<float>(w, "tok.conv_w"); sp.conv_b = hptr<float>(w, "tok.conv_b");
    int rc = ITA_OK;
    // a float-FFN layer gets the attention image only: its FFN is ita_ffn_f32_kernel (no simg_enc / simg_tok)
    const bool lns = !L.ffn_f32 && sp.n1w && sp.n1b && sp.n2w && sp.n2b && stream_range_ok(sp, hdr.E, true, L.ascal, L.fscal);
    if (!stream_range_ok(sp, hdr.E, false, L.ascal, L.fscal)) continue;   // no images: this layer runs on the block kernels
    L.fast_sites = fast_sites_of(L.ascal);
    prove_fused(L, sp, hdr.E, lns);
    const int* fc = L.fused ? L.fused_c : nullptr;
    if (hdr.E == 64) {
      rc = build_stream_image<64, false, false>(sp, L.simg_mha);
      if (!rc && lns) rc = build_stream_image<64, true, false>(sp, L.simg_enc);
      if (!rc && lns && i == 0 && sp.tlw && sp.tlb && sp.conv_w && sp.conv_b) rc = build_stream_image<64, true, true>(sp, L.simg_tok);
      if (!rc && fc) rc = build_stream_image<64, false, false>(sp, L.fimg_mha, fc);
      if (!rc && fc && L.simg_enc) rc = build_stream_image<64, true, false>(sp, L.fimg_enc, fc);
      if (!rc && fc && L.simg_tok) rc = build_stream_image<64, true, true>(sp, L.fimg_tok, fc);
    } else {
      rc = build_stream_image<128, false, false>(sp, L.simg_mha);
      if (!rc && lns) rc = build_stream_image<128, true, false>(sp, L.simg_enc);
      if (!rc && fc) rc = build_stream_image<128, false, false>(sp, L.fimg_mha, fc);
      if (!rc && fc && L.simg_enc) rc = build_stream_image<128, true, false>(sp, L.fimg_enc, fc);
    }
    if (rc) return rc;
  }
  return ITA_OK;
}
#undef NM

// step 4: the LDS images of ita_tok_stream_kernel<E, U8>, when the blob has the conv weights, the bias and the LayerNorm
struct TokHostParams { const float *cw, *cb, *lw, *lb; };
template <int E, bool U8>
void build_tokenizer_image(const TokHostParams& p, char* im) {
  using L = ItaTokStreamLds<E, U8>;
  memcpy(im + L::LNP, p.lw, E * 4); memcpy(im + L::LNP + E * 4, p.lb, E * 4);
  if constexpr (U8) {
    build_tok_tab<E>(p.cw, p.cb, im + L::CW);
  } else {   // the conv weights as they are, as v_mfma_f32_16x16x4_f32 A fragments
    float* cwf = (float*)(im + L::CW);
    for (int st = 0; st < 13; ++st)
      for (int ct = 0; ct < L::NCT; ++ct)
        for (int lane = 0; lane < 64; ++lane) {
          const int t = 4 * st + (lane >> 4), rho = lane & 15, ch = (E / 4) * (rho >> 2) + 4 * ct + (rho & 3);
          cwf[(st * L::NCT + ct) * 64 + lane] = t < 49 ? p.cw[(size_t)ch * 49 + t] : 0.0f;
        }
    memcpy(im + L::CB, p.cb, E * 4);
  }
  fill_tok_taps(im + L::TAP);
}
int build_tokenizer_images(Weights& w) {
  const TokHostParams p{hptr<float>(w, "tok.conv_w"), hptr<float>(w, "tok.conv_b"), hptr<float>(w, "tok.ln_w"), hptr<float>(w, "tok.ln_b")};
  if (!p.cw || !p.cb || !p.lw || !p.lb) return ITA_OK;
  return with_E(w.hdr.E, [&](auto e) -> int {
    constexpr int E = decltype(e)::value;
    // [0]: u8 frames (integer conv tables), [1]: f32 frames (f32 MFMA A fragments); each padded to the larger of the two
    constexpr size_t one8 = ItaTokStreamLds<E, true>::IMAGE, onef = ItaTokStreamLds<E, false>::IMAGE;
    constexpr size_t one = ((one8 > onef ? one8 : onef) + 15) & ~(size_t)15;
    std::vector<char> im(2 * one, 0);
    build_tokenizer_image<E, true>(p, im.data());
    build_tokenizer_image<E, false>(p, im.data() + one);
    w.tok_simg_bytes = one;
    HIPCHK(w.tok_simg.upload(im.data(), im.size()));
    return ITA_OK;
  });
}

// step 5: the exact-f32 fusion tail's conv3x3 weights re-laid [c][ky][kx][o -> 12], so one tap's 9 output weights are contiguous
int build_tail_weights(Weights& w) {
  const float* cw = hptr<float>(w, "tail.conv_w");
  if (!cw) return ITA_OK;
  const int cin = w.hdr.E / 4 + w.hdr.E;
  std::vector<float> wT((size_t)cin * 9 * 12, 0.0f);
  for (int o = 0; o < 9; ++o)
    for (int c = 0; c < cin; ++c)
      for (int k = 0; k < 9; ++k) wT[((size_t)c * 9 + k) * 12 + o] = cw[((size_t)o * cin + c) * 9 + k];
  HIPCHK(w.tail_wT.upload(wT.data(), wT.size()));
  return ITA_OK;
}

// step 6: LSTM [W_ih | W_hh] concatenated along k (layer 0 zero padded to K0P) and b_ih + b_hh for the exact-f32 path,
// and the split-precision A fragments of the LSTM kernels
int build_lstm_weights(Weights& w) {
  if (!hptr<float>(w, "lstm.w_ih0")) return ITA_OK;
  for (int l = 0; l < 3; ++l) {
    char a[32], b[32], ci[32], d[32];
    snprintf(a, sizeof a, "lstm.w_ih%d", l); snprintf(b, sizeof b, "lstm.w_hh%d", l);
    snprintf(ci, sizeof ci, "lstm.b_ih%d", l); snprintf(d, sizeof d, "lstm.b_hh%d", l);
    const float *wih = hptr<float>(w, a), *whh = hptr<float>(w, b), *bih = hptr<float>(w, ci), *bhh = hptr<float>(w, d);
    if (!wih || !whh || !bih || !bhh) return fail(ITA_ERR_BAD_BLOB, "incomplete LSTM parameters");
    const int in = l == 0 ? 517 : 128, kp = l == 0 ? K0P : 256;
    std::vector<float> wc((size_t)512 * kp, 0.0f), bs(512);
    for (int j = 0; j < 512; ++j) {
      memcpy(&wc[(size_t)j * kp], wih + (size_t)j * in, sizeof(float) * in);
      memcpy(&wc[(size_t)j * kp + in], whh + (size_t)j * 128, sizeof(float) * 128);
      bs[j] = bih[j] + bhh[j];
    }
    HIPCHK(w.wcat[l].upload(wc.data(), wc.size()));
    HIPCHK(w.bsum[l].upload(bs.data(), bs.size()));
    // split-precision planes, rows permuted to r' = ut*32 + gate*8 + u so that one MFMA tile holds
    // i,f,g,o of 8 units.  Layers 1, 2: the concatenated [W_ih | W_hh].  Layer 0: only what the folded
    // GEMM does not cover, [W_hh0 (128) | W_ih0[:,512] (desvel) | W_ih0[:,513:517] (quat) | 0] (K0S wide).
    const int kf = l == 0 ? K0S : 256;
    std::vector<float> wf((size_t)512 * kf, 0.0f);
    for (int rp = 0; rp < 512; ++rp) {
      const int j = ((rp >> 3) & 3) * 128 + (rp >> 5) * 8 + (rp & 7);
      if (l == 0) {
        memcpy(&wf[(size_t)rp * kf], whh + (size_t)j * 128, sizeof(float) * 128);
        memcpy(&wf[(size_t)rp * kf + 128], wih + (size_t)j * 517 + 512, sizeof(float) * 5);
      } else {
        memcpy(&wf[(size_t)rp * kf], &wc[(size_t)j * kp], sizeof(float) * 256);
      }
    }
    // ... and stored as the A fragments the LSTM kernels load: [ut][k-range][k-step][lane (row r, k half h)][8]
    const int nsw = l == 0 ? 1 : 4, nss = l == 0 ? kf / 16 : 4;   // k-ranges (one per wave) x k-steps of 16
    std::vector<float> wfrag(wf.size());
    for (int ut = 0; ut < 16; ++ut)
      for (int kw = 0; kw < nsw; ++kw)
        for (int st = 0; st < nss; ++st)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j)
              wfrag[((((size_t)ut * nsw + kw) * nss + st) * 64 + lane) * 8 + j] =
                  wf[(size_t)(ut * 32 + (lane & 31)) * kf + (kw * nss + st) * 16 + 8 * (lane >> 5) + j];
    const int rc = split_upload(wfrag, w.lw_hi[l], w.lw_lo[l], &w.lw_inv_scale[l]);
    if (rc) return rc;
  }
  return ITA_OK;
}

// step 7, device part: Wfold^T [K][512] (K = 128 E) in hmt and the folded bias in hb.  With a fusion tail, unit impulses
// go through the exact f32 kernels, bias-free (PixelShuffle/Upsample/concat/conv3x3, then the decoder Linear), and
// dec(tail(0)) is the bias; without one (models/ITA/QAT/model.py:80-81: the decoder reads the flattened tokens) Wfold is
// the decoder matrix itself.  Then one fold further, since the decoder output feeds only LSTM layer 0:
//   G0^T[k][j] = sum_n Wfold^T[k][n] * W_ih0[j][n]        (wcat[0] holds W_ih0 in its first 517 columns)
int fold_matrix(const Weights& w, int num_cus, std::vector<float>& hmt, std::vector<float>& hb) {
  const int CH = 1024, KFOLD = w.kfold;
  const bool has_tail = w.hdr.has_tail != 0;
  DevBuf<float> imp, feat, mt, zero;
  HIPCHK(imp.alloc((size_t)(has_tail ? CH : 512) * KFOLD));
  HIPCHK(feat.alloc((size_t)CH * 4608));
  HIPCHK(mt.alloc((size_t)KFOLD * 512));
  HIPCHK(zero.alloc(16));
  HIPCHK(hipMemset(zero, 0, sizeof(float) * 16));
  int rc = ITA_OK;
  if (has_tail) {
    auto tail = [&](const float* bias, int B) { return launch_tail(num_cus, w.hdr.E, w.tail_wT, bias, imp, feat, 4608, B, nullptr); };
    for (int c0 = 0; c0 < KFOLD; c0 += CH) {   // bias-free pass: column i of Wfold = dec_nobias(tail_nobias(e_i))
      const size_t n = (size_t)CH * KFOLD;
      if ((rc = launch<ita_impulse_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), nullptr, imp, CH, KFOLD, c0))) return rc;
      if ((rc = tail(zero, CH))) return rc;
      if ((rc = launch_gemm(feat, 4608, w.dec_w, 4608, nullptr, mt + (size_t)c0 * 512, 512, CH, 512, 4608, nullptr))) return rc;
    }
    // bias' = dec(tail(0)) with the real biases
    HIPCHK(hipMemset(imp, 0, sizeof(float) * KFOLD));
    if ((rc = tail(w.tail_b, 1))) return rc;
    if ((rc = launch_gemm(feat, 4608, w.dec_w, 4608, w.dec_b, imp, 512, 1, 512, 4608, nullptr))) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(hb.data(), imp, 512 * sizeof(float), hipMemcpyDeviceToHost));
  } else {
    // Wfold^T[k][n] = dec_w[n][k]: transposed on the host (once, at load time); bias' = the decoder bias
    const float *dw = hptr<float>(w, "dec.w"), *db = hptr<float>(w, "dec.b");
    for (int n = 0; n < 512; ++n)
      for (int k = 0; k < KFOLD; ++k) hmt[(size_t)k * 512 + n] = dw[(size_t)n * KFOLD + k];
    HIPCHK(hipMemcpy(mt, hmt.data(), hmt.size() * sizeof(float), hipMemcpyHostToDevice));
    memcpy(hb.data(), db, 512 * sizeof(float));
  }
  // computed with the exact f32 GEMM; the buffer that held the impulses is reused for the result
  if ((rc = launch_gemm(mt, 512, w.wcat[0], K0P, nullptr, imp, 512, KFOLD, 512, 512, nullptr))) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(hmt.data(), imp, hmt.size() * sizeof(float), hipMemcpyDeviceToHost));
  return ITA_OK;
}

// step 7: the folded tail + decoder + W_ih0 matrix as split-precision planes, and its bias
int build_fold(Weights& w, int num_cus) {
  const int KFOLD = w.kfold, LDFOLD = w.ldfold;
  std::vector<float> hmt((size_t)KFOLD * 512), hb(512);
  int rc = fold_matrix(w, num_cus, hmt, hb);   // (its device temporaries are gone before the planes are allocated)
  if (rc) return rc;
  // rows of the GEMM weight in the permuted gate order r' = ut*32 + gate*8 + u (ita_lstm_head_kernel.h)
  std::vector<float> wf((size_t)512 * LDFOLD, 0.0f);
  for (int rp = 0; rp < 512; ++rp) {
    const int j = ((rp >> 3) & 3) * 128 + (rp >> 5) * 8 + (rp & 7);
    for (int k = 0; k < KFOLD; ++k) wf[(size_t)rp * LDFOLD + k] = hmt[(size_t)k * 512 + j];
  }
  if ((rc = split_upload(wf, w.fold_hi, w.fold_lo, &w.fold_inv_scale))) return rc;
  {
    // the same values in fragment order for ita_gemm_f16x3_tiny_kernel (same scale: max |w| is the same)
    std::vector<float> wfr((size_t)512 * KFOLD);
    for (int nt = 0; nt < 32; ++nt)
      for (int st = 0; st < KFOLD / 32; ++st)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j)
            wfr[(((size_t)nt * (KFOLD / 32) + st) * 64 + lane) * 8 + j] =
                wf[(size_t)(nt * 16 + (lane & 15)) * LDFOLD + st * 32 + 8 * (lane >> 4) + j];
    float inv2 = 0.0f;
    if ((rc = split_upload(wfr, w.foldf_hi, w.foldf_lo, &inv2))) return rc;
    if (inv2 != w.fold_inv_scale) return fail(ITA_ERR_UNSUPPORTED, "fragment copy of the folded weights got a different scale");
  }
  // bias'' = W_ih0[:, :512] . bias' + b_ih0 + b_hh0   (gate-major order)
  const float *wih0 = hptr<float>(w, "lstm.w_ih0"), *bih0 = hptr<float>(w, "lstm.b_ih0"), *bhh0 = hptr<float>(w, "lstm.b_hh0");
  std::vector<float> b2(512);
  for (int j = 0; j < 512; ++j) {
    double acc = (double)bih0[j] + (double)bhh0[j];
    for (int n = 0; n < 512; ++n) acc += (double)wih0[(size_t)j * 517 + n] * (double)hb[n];
    b2[j] = (float)acc;
  }
  HIPCHK(w.fold_bias.upload(b2.data(), b2.size()));
  w.folded = true;
  return ITA_OK;
}

}  // namespace
