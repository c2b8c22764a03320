// C ABI (include/thewhisper.h) + context + kernel orchestration for the MI355X Whisper hot path.
// Host-side control only: every FLOP/byte of the path runs in the gfx950 kernels of k_*.hip.
#include "../../include/thewhisper.h"
#include "tw_common.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <chrono>
#include <string>
#include <tuple>
#include <vector>

namespace {

thread_local std::string g_create_error;

struct LayerW {
  void *ln1_g = nullptr, *ln1_b = nullptr;  // self_attn_layer_norm
  void *wqkv = nullptr, *bqkv = nullptr;    // [3d, d], [3d] (q rows pre-scaled by 1/8, k bias = 0)
  // MXFP8 contexts: block scales of the six decoder projections (inside the weight buffers, behind the fp8 fragments)
  unsigned char *s_qkv = nullptr, *s_o = nullptr, *s_qc = nullptr, *s_oc = nullptr, *s_1 = nullptr, *s_2 = nullptr;
  void *wo = nullptr, *bo = nullptr;
  void *lnx_g = nullptr, *lnx_b = nullptr;  // encoder_attn_layer_norm (decoder)
  void *wq_c = nullptr, *bq_c = nullptr;    // cross q (pre-scaled)
  void *wkv_c = nullptr, *bkv_c = nullptr;  // [2d, d] cross k|v
  void *wo_c = nullptr, *bo_c = nullptr;
  void *ln2_g = nullptr, *ln2_b = nullptr;  // final_layer_norm
  void *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
  // folded pre-LayerNorm companions of the decoder's LN'd projections (float32 [N]): see k_decode.hip
  float *qkv_gw = nullptr, *qkv_cb = nullptr, *qc_gw = nullptr, *qc_cb = nullptr, *fc1_gw = nullptr, *fc1_cb = nullptr;
  // weight rows per workgroup tile each decoder projection was laid out for (k_decode.hip: 16, or 8 / 4 for the narrow ones)
  int tr_qkv = 16, tr_o = 16, tr_qc = 16, tr_oc = 16, tr_1 = 16, tr_2 = 16;
};

// ---- pinned host staging: every block has a type, and its fields are the only way in (tw_ctx::h_*; alloc_staging) ----
struct PinnedScratch {       // h_pinned
  int finished[8][64];       // ring of the generate loop's read-backs of the finished flags, one slot per launch
  int n_valid[64];           // tw_logmel's valid-sample counts
  DecState state;            // reset_state's upload
};
struct VerifyStage {         // h_verify: the device's verify_state (tw_common.h: SamplerArgs) as read back, and what a round resets it to
  int first_mismatch, decided, choice[64];   // [0] | [1] = p_acc + 1 once the round is decided, else 0 | [2 + b] = stream b's token there
  int reset[2];                              // the two leading words at the start of a round
};
struct GenStage {            // h_stage: the initial state of a tw_generate_* call; tw_score_tokens stages its suppress lists here too
  int first[64], finished0[64], last_ts0[64];   // per stream: first input token | finished flag | last timestamp token
  int bsup[64], sup[1024];                      // begin-suppress and suppress lists
  DecState state;
  float inv_t[64]; uint32_t key[64][2], off[64][2]; int noisy[64];   // tw_generate_sample
  int top_k[64]; float top_p[64];                                    // tw_generate_sample_filtered
};
struct RowStage { int *tok, *lastts; };                  // h_rows: position-major tables of a rows-mode pass, [row_ids_cap] each (fill_row_tables)
struct ScoreBlock { float *masked, *raw, *no_speech; };  // tw_score_tokens' results, device and pinned alike: [Bmax][P] | [Bmax][P] | [Bmax]

}  // namespace

struct tw_ctx {
  tw_config cfg{};
  int dtype = 1;
  bool w8 = false;   // decoder projection weights in MXFP8 (TW_BF16_MXFP8 / TW_BF16_W8A16 contexts)
  int a16 = 0;       // ... contracted as bf16 after widening in registers (TW_BF16_W8A16)
  // "cross query ahead" (decode_core): the decoder's cross-attention query projection is folded into the two launches before
  // it, which saves one dependent launch per layer and step.  du = float32 [Bmax][d] pre-activation of that projection.
  bool fuse_cq = false;
  bool enc_fold = true;   // encoder pre-LayerNorms folded into the QKV / fc1 GEMMs (GemmEpilogue::stats_*); false: two LayerNorm launches per layer
  float *ln_stats_a = nullptr, *ln_stats_b = nullptr;   // [rows][d / 32][2] partial row statistics of xa / xb
  float* du = nullptr;
  float* dstats = nullptr;   // [Bmax][d / tile rows][2] partial LayerNorm statistics of the residual stream (see GemvArgs::stats)
  unsigned char* logit_ws = nullptr;  // block scales of logit_w
  size_t esz = 2;
  int d = 0, H = 0, ffn = 0, V = 0, T = 0, Tp = 0, P = 0, C = 0, Bmax = 0, Le = 0, Ld = 0, n_mels = 0, Ha = 0;
  std::string err;
  std::vector<void*> allocs;
  hipStream_t own_stream = nullptr;

  // weights
  void *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr, *conv2_b = nullptr;
  void *enc_pos_raw = nullptr, *enc_pos = nullptr, *enc_ln_g = nullptr, *enc_ln_b = nullptr;
  void *tok_emb = nullptr, *dec_pos = nullptr, *dec_ln_g = nullptr, *dec_ln_b = nullptr;
  void* logit_w = nullptr;  // tok_emb with the final LayerNorm gain folded in (the lookup table itself stays unscaled)
  float *logit_gw = nullptr, *logit_cb = nullptr;
  std::vector<LayerW> enc, dec;
  std::set<std::string> loaded;
  bool finalized = false;
  bool shares_weights = false;   // tw_create_sibling: the weight pointers belong to another context (never freed here)

  // log-mel
  LogmelTables lm{};
  float* logspec_ws = nullptr; size_t logspec_cap = 0;
  unsigned* lm_max = nullptr;
  int* n_valid_dev = nullptr;

  // encoder workspace
  void *melT = nullptr, *h1 = nullptr, *xa = nullptr, *xb = nullptr, *lnbuf = nullptr, *qbuf = nullptr, *kbuf = nullptr,
       *vtbuf = nullptr, *attn = nullptr, *ffnh = nullptr, *enc_out = nullptr;
  int encoded_B = 0, cross_B = 0;

  // decoder state
  void *self_k = nullptr, *self_v = nullptr, *cross_k = nullptr, *cross_v = nullptr;
  unsigned char *cross_ksc = nullptr, *cross_vsc = nullptr;  // MXFP8 contexts: per-key scale bytes of the fp8 cross K / V^T caches [Ld][B][H][Tp]
  void *dx0 = nullptr, *dx1 = nullptr, *dq = nullptr, *datt = nullptr, *dh = nullptr;
  float* logits = nullptr;
  float* align = nullptr;
  int* align_slot = nullptr;  // [Ld][H]
  int *seq = nullptr, *cur_ids = nullptr, *finished = nullptr, *last_ts = nullptr;
  DecState* stt = nullptr;
  int* begin_suppress_dev = nullptr; int* suppress_dev = nullptr;
  SamplerPartial* sampler_partials = nullptr;
  // tw_generate_sample: per-row temperature reciprocals, Philox keys / offsets, noisy flags (uploaded per call) and the slice partials
  float* sample_inv_t = nullptr; uint32_t* sample_key = nullptr; uint32_t* sample_off = nullptr; int* sample_noisy = nullptr;   // [64], [64][2], [64][2], [64]
  SamplePartial* sample_parts = nullptr;   // [64][32]
  // tw_generate_sample_filtered: per-row top-k / top-p (uploaded per call) and the filter kernel's choice
  int* filter_top_k = nullptr; float* filter_top_p = nullptr; int* filter_choice = nullptr;   // [64] each
  unsigned* suppress_bits = nullptr;  // [(V+31)/32] static suppress list as a bitmap, rebuilt per generate call
  PinnedScratch* h_pinned = nullptr;
  int* row_ids = nullptr;   // device token table of a prefill (position-major), row_ids_cap ints
  RowStage h_rows{};        // its pinned host staging, and that of row_lastts
  // draft-and-verify (tw_greedy_opts::n_draft): per-row sampler state and results (SamplerArgs, tw_common.h)
  int* row_lastts = nullptr;     // [row_ids_cap] position-major like row_ids
  int* row_choice = nullptr;     // [row_ids_cap]
  int* verify_state = nullptr;   // [2 + 64] device
  VerifyStage* h_verify = nullptr;
  // tw_generate_greedy_biased: the packed table of the call's sequences (tw_common.h: SeqBiasArgs) and its pinned staging, both of
  // kSeqBiasTabWords words, allocated by the first biased call of the context
  int* bias_tab = nullptr; int* h_bias = nullptr;
  // tw_generate_greedy_repeat: the per-stream table (tw_common.h: RepeatArgs) of kRepeatTabWords words and its pinned staging, allocated
  // by the first call of the context that sets a penalty or an n-gram size
  int* repeat_tab = nullptr; int* h_repeat = nullptr;
  // tw_generate_greedy_ragged: the per-stream padding lengths [64] the ragged kernels read (tw_common.h: tw_row_pos) and their pinned
  // staging, allocated by the first ragged call of the context
  int* n_pad_tab = nullptr; int* h_n_pad = nullptr;
  // tw_detect_language: ids [kLangMax] | out ids [Bmax] | out probabilities [Bmax][kLangMax] | the step's input ids [Bmax], on the device
  // and pinned, allocated by the first call of the context
  int* lang_tab = nullptr; int* h_lang = nullptr;
  // tw_generate_beam: the state tables of the call (BeamTab: scores, finished set, flags, penalty table, finished hypotheses), their
  // pinned image (up with the initial state, down with the result) and the slice partials, allocated by the first beam call of the context
  int* beam_tab = nullptr; int* h_beam = nullptr; BeamPartial* beam_parts = nullptr;
  // tw_generate_beam_aligned: the ancestry of the alignment rows (BeamArgs::back [512][64], then fin_last [64]), allocated by the first
  // such call with want_alignment
  int* beam_anc = nullptr;
  int last_draft[4] = {0, 0, 0, 0};   // of the last greedy call: tokens offered, accepted, verify launches, verify rounds
  int last_prompt_rows[2] = {0, 0};   // of the last call of the generate family: rows launches its prompt took, positions they consumed
  size_t row_ids_cap = 0;
  // tw_score_tokens: its own token table, processor tables, slice partials and results, so that nothing a later tw_generate_greedy
  // (or its captured step graphs) reads is touched
  int* score_seq = nullptr;            // [Bmax][P]
  int *score_bsup = nullptr, *score_sup = nullptr;   // [64], [1024]
  unsigned* score_bits = nullptr;      // [(V+31)/32]
  ScorePartial* score_parts = nullptr; // [64][32]
  ScoreBlock score_out{}, h_score{}; size_t score_floats = 0;   // one block of score_floats floats each, on the device and pinned (masked = its start)
  int row_cap = 0;          // rows the per-token activation buffers hold (>= max_batch; 64 for the prefill launches)
  GenStage* h_stage = nullptr;
  int* h_seq = nullptr;     // pinned token table [Bmax][P] of tw_generate_* (up and down) and tw_score_tokens (up)
  hipEvent_t ring_ev[8]{};
  int last_seq_len = 0, last_n_prompt = 0;
  int dec_key_bound = 0;  // upper bound of decoder positions for the current decode (prompt + max new tokens)
  int enc_pos_rows = 0;  // rows of the encoder positional table as loaded (1500 upstream)

  // dtw workspace
  float *zbuf = nullptr, *mat = nullptr, *out_ts = nullptr;
  signed char* trace = nullptr;
  int* n_cols = nullptr;
  int* dtw_len = nullptr;   // tw_token_timestamps_each: the streams' lengths [Bmax], allocated by its first call

  // graph replay of one decode step
  // one captured step per 64-key bucket of the self-attention length (the step at position s only has to read keys
  // [0, roundup(s + 1, 64)), and the host knows s): fewer bytes per step than one graph sized for the longest sequence
  std::map<std::string, hipGraphExec_t> step_graphs;
  std::string step_graph_key;

  // timing
  hipEvent_t ev0[5]{}, ev1[5]{};
  bool ev_valid[5]{};
  int last_steps = 0;
};

namespace {

int fail(tw_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(c, expr)                                                                       \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail((c), TW_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

template <typename P>
int dalloc(tw_ctx* c, P** p, size_t bytes, bool zero) {
  void* q = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(c, TW_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  c->allocs.push_back(q);
  if (zero) {
    e = hipMemset(q, 0, bytes);
    if (e != hipSuccess) return fail(c, TW_EHIP, "hipMemset failed: %s", hipGetErrorString(e));
  }
  *p = reinterpret_cast<P*>(q);
  return TW_OK;
}
#define ALLOC(c, ptr, bytes, zero)                   \
  do {                                               \
    int _r = dalloc((c), &(ptr), (bytes), (zero));   \
    if (_r != TW_OK) return _r;                      \
  } while (0)

inline hipStream_t pick_stream(tw_ctx* c, void* s) { return s ? reinterpret_cast<hipStream_t>(s) : c->own_stream; }

// Every entry point runs with the context's device current and restores the caller's device on exit: worker threads
// (BatchingHub, the gateway's thread pool, the reference scheduler's thread) start on device 0, and kernel launches,
// memcpys and hipMalloc go to the calling thread's CURRENT device, not to the device a stream belongs to.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define TW_ON_DEVICE(c) DeviceGuard _tw_guard((c)->cfg.device)

char* at(void* base, size_t elems, size_t esz) { return reinterpret_cast<char*>(base) + elems * esz; }

// slaney mel bank, float64 (HF:audio_utils.py:638-729), then cast to float32 as the reference does
void build_mel_bank(int n_mels, std::vector<float>& bank, std::vector<int>& lo, std::vector<int>& hi) {
  const int nb = 201;
  auto hz2mel = [](double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; };
  auto mel2hz = [](double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; };
  const double mmin = hz2mel(0.0), mmax = hz2mel(8000.0);
  std::vector<double> ff(n_mels + 2);
  for (int i = 0; i < n_mels + 2; ++i) ff[i] = mel2hz(mmin + (mmax - mmin) * (double)i / (double)(n_mels + 1));
  bank.assign((size_t)nb * n_mels, 0.f);
  lo.assign(n_mels, nb);
  hi.assign(n_mels, 0);
  for (int k = 0; k < nb; ++k) {
    const double fk = 8000.0 * (double)k / (double)(nb - 1);
    for (int m = 0; m < n_mels; ++m) {
      const double down = -(ff[m] - fk) / (ff[m + 1] - ff[m]);
      const double up = (ff[m + 2] - fk) / (ff[m + 2] - ff[m + 1]);
      double v = std::fmax(0.0, std::fmin(down, up));
      v *= 2.0 / (ff[m + 2] - ff[m]);
      const float vf = (float)v;
      bank[(size_t)k * n_mels + m] = vf;
      if (vf != 0.f) {
        if (k < lo[m]) lo[m] = k;
        if (k + 1 > hi[m]) hi[m] = k + 1;
      }
    }
  }
  for (int m = 0; m < n_mels; ++m)
    if (hi[m] == 0) lo[m] = 0;
}

// Every pinned staging block of a context and tw_score_tokens' device results: the one place that knows a capacity or where a
// part begins (needs Bmax, P and row_ids_cap).  Freed in tw_destroy.
int alloc_staging(tw_ctx* c) {
  const size_t plane = (size_t)c->Bmax * c->P;
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_pinned), sizeof(PinnedScratch), hipHostMallocDefault));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_verify), sizeof(VerifyStage), hipHostMallocDefault));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_stage), sizeof(GenStage), hipHostMallocDefault));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_seq), sizeof(int) * plane, hipHostMallocDefault));
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_rows.tok), sizeof(int) * 2 * c->row_ids_cap, hipHostMallocDefault));
  c->h_rows.lastts = c->h_rows.tok + c->row_ids_cap;
  c->score_floats = 2 * plane + c->Bmax;
  ALLOC(c, c->score_out.masked, sizeof(float) * c->score_floats, true);
  HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_score.masked), sizeof(float) * c->score_floats, hipHostMallocDefault));
  for (ScoreBlock* s : {&c->score_out, &c->h_score}) { s->raw = s->masked + plane; s->no_speech = s->raw + plane; }
  return TW_OK;
}

void tic(tw_ctx* c, int i, hipStream_t st) { (void)hipEventRecord(c->ev0[i], st); }
void toc(tw_ctx* c, int i, hipStream_t st) { (void)hipEventRecord(c->ev1[i], st); c->ev_valid[i] = true; }

}  // namespace

extern "C" {

const char* tw_version(void) { return TW_VERSION_STRING; }

const char* tw_last_error(const tw_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int tw_destroy(tw_ctx* c) {
  if (!c) return TW_OK;
  TW_ON_DEVICE(c);
  (void)hipDeviceSynchronize();
  for (auto& kv : c->step_graphs) (void)hipGraphExecDestroy(kv.second);
  for (void* p : c->allocs) (void)hipFree(p);
  void* const pinned[] = {c->h_pinned, c->h_stage, c->h_seq, c->h_rows.tok, c->h_verify, c->h_score.masked, c->h_bias, c->h_repeat, c->h_n_pad, c->h_beam, c->h_lang};
  for (void* p : pinned)
    if (p) (void)hipHostFree(p);
  for (int i = 0; i < 5; ++i) {
    if (c->ev0[i]) (void)hipEventDestroy(c->ev0[i]);
    if (c->ev1[i]) (void)hipEventDestroy(c->ev1[i]);
  }
  for (int i = 0; i < 8; ++i)
    if (c->ring_ev[i]) (void)hipEventDestroy(c->ring_ev[i]);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return TW_OK;
}

static int create_ctx(const tw_config* cfg, const tw_ctx* share, tw_ctx** out);

int tw_create(const tw_config* cfg, tw_ctx** out) { return create_ctx(cfg, nullptr, out); }

int tw_create_sibling(const tw_ctx* src, int32_t max_batch, tw_ctx** out) {
  if (!src || !out) return fail(nullptr, TW_EINVAL, "tw_create_sibling: null argument");
  if (!src->finalized) return fail(nullptr, TW_ESTATE, "tw_create_sibling: the source context's weights are not finalized");
  if (src->shares_weights) return fail(nullptr, TW_EINVAL, "tw_create_sibling: the source is itself a sibling (create it from the owner)");
  tw_config cfg = src->cfg;
  cfg.max_batch = max_batch;
  return create_ctx(&cfg, src, out);
}

// share != nullptr: every weight pointer is taken from `share` (finalized; it owns them and must outlive this context) instead
// of being allocated; workspace, arenas, streams, events and graphs are this context's own
static int create_ctx(const tw_config* cfg, const tw_ctx* share, tw_ctx** out) {
  if (!cfg || !out) return fail(nullptr, TW_EINVAL, "tw_create: null argument");
  *out = nullptr;
  if (cfg->heads <= 0 || cfg->d_model != cfg->heads * 64)
    return fail(nullptr, TW_EINVAL, "head_dim must be 64 (d_model=%d heads=%d)", cfg->d_model, cfg->heads);
  if (cfg->dtype != TW_BF16 && cfg->dtype != TW_F32 && cfg->dtype != TW_F16 && cfg->dtype != TW_BF16_MXFP8 && cfg->dtype != TW_BF16_W8A16)
    return fail(nullptr, TW_EINVAL, "dtype must be TW_BF16, TW_F16, TW_F32, TW_BF16_MXFP8 or TW_BF16_W8A16");
  const bool cfg_w8 = cfg->dtype == TW_BF16_MXFP8 || cfg->dtype == TW_BF16_W8A16;
  if (cfg_w8 && (cfg->d_model % 128 || cfg->ffn % 128))
    return fail(nullptr, TW_EINVAL, "TW_BF16_MXFP8 / TW_BF16_W8A16 need d_model and ffn to be multiples of 128");
  if (cfg->d_model % 64 || cfg->ffn % 64 || cfg->d_model > 1280)
    return fail(nullptr, TW_EINVAL, "d_model/ffn must be multiples of 64 and d_model <= 1280");
  if (cfg->max_batch < 1 || cfg->max_batch > 64) return fail(nullptr, TW_EINVAL, "max_batch must be in [1,64]");
  if (cfg->dtype == TW_BF16_MXFP8 && cfg->max_batch > 16)
    return fail(nullptr, TW_EINVAL, "TW_BF16_MXFP8: max_batch must be in [1,16] (TW_BF16_W8A16 takes up to 64 streams)");
  if (cfg->source_positions < 8 || cfg->source_positions > 1500 || cfg->target_positions < 8 || cfg->target_positions > 511)
    return fail(nullptr, TW_EINVAL, "source_positions must be in [8,1500], target_positions in [8,511]");
  if (cfg->n_align_heads < 0 || cfg->n_align_heads > TW_MAX_ALIGN_HEADS) return fail(nullptr, TW_EINVAL, "bad n_align_heads");
  if (cfg->n_mels < 1 || cfg->n_mels > 256) return fail(nullptr, TW_EINVAL, "bad n_mels");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, TW_EHIP, "no HIP device available (the MI355X path has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, TW_EINVAL, "device %d out of range", cfg->device);
  DeviceGuard guard(cfg->device);   // allocations below land on the context's device; the caller's device is restored on return
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) return fail(nullptr, TW_EHIP, "hipSetDevice(%d) failed", cfg->device);

  tw_ctx* c = new tw_ctx();
  c->cfg = *cfg;
  c->w8 = cfg_w8;
  c->a16 = cfg->dtype == TW_BF16_W8A16;
  c->dtype = c->w8 ? (int)TW_BF16 : cfg->dtype;
  c->esz = c->dtype == TW_F32 ? 4 : 2;
  c->d = cfg->d_model; c->H = cfg->heads; c->ffn = cfg->ffn; c->V = cfg->vocab;
  c->T = cfg->source_positions; c->Tp = (c->T + 63) / 64 * 64; c->P = cfg->target_positions;
  c->n_mels = cfg->n_mels; c->C = (cfg->n_mels + 63) / 64 * 64;
  c->Bmax = cfg->max_batch; c->Le = cfg->enc_layers; c->Ld = cfg->dec_layers; c->Ha = cfg->n_align_heads;
  c->fuse_cq = c->d == c->H * 64;
  c->enc_fold = c->d % 64 == 0 && c->d <= 1280;   // (k_gemm.hip: TW_LN_HALF partial statistics per thread)
  auto bail = [&](int r) { g_create_error = c->err; tw_destroy(c); return r; };
#define CALLOC(ptr, bytes, zero) do { int _r = dalloc(c, &(ptr), (bytes), (zero)); if (_r != TW_OK) return bail(_r); } while (0)
#define CHIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { fail(c, TW_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); return bail(TW_EHIP); } } while (0)
  CHIP(hipStreamCreate(&c->own_stream));
  for (int i = 0; i < 5; ++i) { CHIP(hipEventCreate(&c->ev0[i])); CHIP(hipEventCreate(&c->ev1[i])); }
  for (int i = 0; i < 8; ++i) CHIP(hipEventCreateWithFlags(&c->ring_ev[i], hipEventDisableTiming));

  const size_t e = c->esz;
  const size_t d = c->d, H = c->H, F = c->ffn, V = c->V, T = c->T, Tp = c->Tp, P = c->P, C = c->C, B = c->Bmax;
  if (share) {
    c->shares_weights = true;
    c->fuse_cq = share->fuse_cq;
    c->enc_fold = share->enc_fold;
    c->a16 = share->a16;
    c->conv1_w = share->conv1_w; c->conv1_b = share->conv1_b; c->conv2_w = share->conv2_w; c->conv2_b = share->conv2_b;
    c->enc_pos_raw = share->enc_pos_raw; c->enc_pos = share->enc_pos; c->enc_ln_g = share->enc_ln_g; c->enc_ln_b = share->enc_ln_b;
    c->tok_emb = share->tok_emb; c->dec_pos = share->dec_pos; c->dec_ln_g = share->dec_ln_g; c->dec_ln_b = share->dec_ln_b;
    c->logit_w = share->logit_w; c->logit_gw = share->logit_gw; c->logit_cb = share->logit_cb; c->logit_ws = share->logit_ws;
    c->enc = share->enc; c->dec = share->dec;
    c->loaded = share->loaded; c->enc_pos_rows = share->enc_pos_rows; c->finalized = true;
  } else {
  // ---- weights ----
  CALLOC(c->conv1_w, d * 3 * C * e, true);
  CALLOC(c->conv1_b, d * e, true);
  CALLOC(c->conv2_w, d * 3 * d * e, true);
  CALLOC(c->conv2_b, d * e, true);
  CALLOC(c->enc_pos_raw, (size_t)1500 * d * 4, true);
  CALLOC(c->enc_pos, T * d * e, true);
  CALLOC(c->enc_ln_g, d * e, true);
  CALLOC(c->enc_ln_b, d * e, true);
  CALLOC(c->tok_emb, V * d * e, true);
  CALLOC(c->dec_pos, P * d * e, true);
  CALLOC(c->dec_ln_g, d * e, true);
  CALLOC(c->dec_ln_b, d * e, true);
  CALLOC(c->logit_w, ((V + 15) / 16 * 16) * d * e, false);  // padded to whole 16-row tiles
  CALLOC(c->logit_gw, V * 4, true);
  CALLOC(c->logit_cb, V * 4, true);
  c->enc.resize(c->Le);
  c->dec.resize(c->Ld);
  auto alloc_layer = [&](LayerW& L, bool decoder) -> int {
    int r;
#define LA(ptr, n) if ((r = dalloc(c, &(ptr), (n) * e, true)) != TW_OK) return r
    // decoder with "cross query ahead": a fourth block of rows behind q|k|v (the folded cross-query weight) and a second one
    // behind the out-projection (cross-query weight . out-projection), see tw_finalize_weights
    const size_t qkv_blocks = (decoder && c->fuse_cq) ? 4 : 3, o_blocks = (decoder && c->fuse_cq) ? 2 : 1;
    LA(L.ln1_g, d); LA(L.ln1_b, d); LA(L.wqkv, qkv_blocks * d * d); LA(L.bqkv, 3 * d); LA(L.wo, o_blocks * d * d); LA(L.bo, d);
    LA(L.ln2_g, d); LA(L.ln2_b, d); LA(L.w1, F * d); LA(L.b1, F); LA(L.w2, d * F); LA(L.b2, d);
    if (!decoder && c->enc_fold) {
      if ((r = dalloc(c, &L.qkv_gw, 3 * d * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.qkv_cb, 3 * d * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.fc1_gw, F * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.fc1_cb, F * 4, true)) != TW_OK) return r;
    }
    if (decoder) {
      if ((r = dalloc(c, &L.qkv_gw, 4 * d * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.qkv_cb, 4 * d * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.qc_gw, d * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.qc_cb, d * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.fc1_gw, F * 4, true)) != TW_OK) return r;
      if ((r = dalloc(c, &L.fc1_cb, F * 4, true)) != TW_OK) return r;
      LA(L.lnx_g, d); LA(L.lnx_b, d); LA(L.wq_c, d * d); LA(L.bq_c, d); LA(L.wkv_c, 2 * d * d); LA(L.bkv_c, 2 * d);
      LA(L.wo_c, d * d); LA(L.bo_c, d);
    }
#undef LA
    return TW_OK;
  };
  for (auto& L : c->enc) { int r = alloc_layer(L, false); if (r != TW_OK) return bail(r); }
  for (auto& L : c->dec) { int r = alloc_layer(L, true); if (r != TW_OK) return bail(r); }
  }  // !share

  // ---- log-mel tables ----
  {
    std::vector<double> tw(400), win(400);
    const double two_pi = 6.283185307179586476925286766559;
    for (int j = 0; j < 400; ++j) { tw[j] = std::cos(two_pi * j / 400.0); win[j] = 0.5 - 0.5 * std::cos(two_pi * j / 400.0); }
    std::vector<float> bank; std::vector<int> lo, hi;
    build_mel_bank(c->n_mels, bank, lo, hi);
    double *dtw_ = nullptr, *dwin = nullptr; float* dbank = nullptr; int *dlo = nullptr, *dhi = nullptr;
    CALLOC(dtw_, 400 * 8, false); CALLOC(dwin, 400 * 8, false); CALLOC(dbank, bank.size() * 4, false);
    CALLOC(dlo, lo.size() * 4, false); CALLOC(dhi, hi.size() * 4, false);
    CHIP(hipMemcpy(dtw_, tw.data(), 400 * 8, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(dwin, win.data(), 400 * 8, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(dbank, bank.data(), bank.size() * 4, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(dlo, lo.data(), lo.size() * 4, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(dhi, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
    c->lm = LogmelTables{dtw_, dwin, dbank, dlo, dhi};
    c->logspec_cap = B * (size_t)c->n_mels * (2 * T);
    CALLOC(c->logspec_ws, c->logspec_cap * 4, false);
    CALLOC(c->lm_max, B * 4, true);
    CALLOC(c->n_valid_dev, B * 4, true);
  }
  // ---- encoder workspace ----
  CALLOC(c->melT, B * (2 * T + 2) * C * e, true);
  CALLOC(c->h1, B * (2 * T + 2) * d * e, true);   // pad rows 0 and 2T+1 of every clip stay zero
  CALLOC(c->xa, B * T * d * e, false);
  CALLOC(c->xb, B * T * d * e, false);
  CALLOC(c->lnbuf, B * T * d * e, false);
  CALLOC(c->ln_stats_a, B * T * (d / 32) * 8, false);
  CALLOC(c->ln_stats_b, B * T * (d / 32) * 8, false);
  CALLOC(c->qbuf, B * T * d * e, false);
  CALLOC(c->kbuf, B * T * d * e, false);
  CALLOC(c->vtbuf, B * H * 64 * Tp * e, true);      // key padding [T, Tp) stays zero
  CALLOC(c->attn, B * T * d * e, false);
  CALLOC(c->ffnh, B * T * F * e, false);
  CALLOC(c->enc_out, B * T * d * e, false);
  // ---- decoder state ----
  const size_t Ld = c->Ld;
  // decoder K / V^T caches: fragment-major per (stream, head), key count padded to 64 (tw_kf_index / tw_vtf_index);
  // the padding is never written and must stay zero (V^T padding meets probability 0 in the P.V product)
  const size_t Pp = (P + 63) / 64 * 64;
  CALLOC(c->self_k, Ld * B * Pp * d * e, true);
  CALLOC(c->self_v, Ld * B * Pp * d * e, true);
  // cross K / V^T: bf16 (f32) fragment-major, or - MXFP8 contexts - e4m3 with one scale byte per (key, head) (tw_common.h)
  const size_t ckv_e = c->w8 ? 1 : e;
  CALLOC(c->cross_k, Ld * B * Tp * d * ckv_e, true);
  CALLOC(c->cross_v, Ld * B * Tp * d * ckv_e, true);
  if (c->w8) {
    CALLOC(c->cross_ksc, Ld * B * H * Tp, true);
    CALLOC(c->cross_vsc, Ld * B * H * Tp, true);
  }
  // per-token decoder activations that feed a projection are fragment-major in groups of 16 streams (tw_xt_index)
  // (sized for the 64 rows of a prefill launch - rows mode, tw_common.h - whatever max_batch is: < 1 MB; rows_per_launch() is at
  //  most 64, so no launch's row count ever has to be clamped to row_cap)
  c->row_cap = (int)std::max<size_t>(B, 64);
  const size_t R = c->row_cap;
  const size_t Bg = (R + 15) / 16 * 16;  // whole groups of 16 streams
  CALLOC(c->dx0, Bg * d * e, true); CALLOC(c->dx1, Bg * d * e, true); CALLOC(c->dq, R * d * e, true);
  CALLOC(c->datt, Bg * d * e, true); CALLOC(c->dh, Bg * F * e, true);
  CALLOC(c->du, R * d * 4, true);
  CALLOC(c->dstats, R * (d / 4) * 2 * 4, true);
  c->row_ids_cap = (size_t)B * P;
  CALLOC(c->row_ids, c->row_ids_cap * 4, true);
  CALLOC(c->row_lastts, c->row_ids_cap * 4, true);
  CALLOC(c->row_choice, c->row_ids_cap * 4, true);
  CALLOC(c->verify_state, (2 + 64) * 4, true);
  CALLOC(c->logits, R * V * 4, true);   // (the rows of a verify launch - up to 64 - whatever max_batch is: 13 MB)
  const size_t Ha = c->Ha > 0 ? c->Ha : 1;
  CALLOC(c->align, B * Ha * P * T * 4, true);
  CALLOC(c->align_slot, Ld * H * 4, false);
  {
    std::vector<int> slots(Ld * H, -1);
    for (int j = 0; j < c->Ha; ++j) {
      const int l = cfg->align_heads[2 * j], h = cfg->align_heads[2 * j + 1];
      if (l < 0 || l >= (int)Ld || h < 0 || h >= (int)H) { fail(c, TW_EINVAL, "alignment head (%d,%d) out of range", l, h); return bail(TW_EINVAL); }
      slots[(size_t)l * H + h] = j;
    }
    CHIP(hipMemcpy(c->align_slot, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
  }
  CALLOC(c->seq, B * P * 4, true); CALLOC(c->cur_ids, B * 4, true); CALLOC(c->finished, B * 4, true);
  CALLOC(c->last_ts, B * 4, true); CALLOC(c->stt, sizeof(DecState), true);
  CALLOC(c->begin_suppress_dev, 64 * 4, true); CALLOC(c->suppress_dev, 1024 * 4, true);
  CALLOC(c->suppress_bits, ((V + 31) / 32 + 2048) * 4, true);
  CALLOC(c->sampler_partials, 64 * 32 * sizeof(SamplerPartial), true);
  CALLOC(c->sample_inv_t, 64 * 4, true); CALLOC(c->sample_key, 128 * 4, true); CALLOC(c->sample_off, 128 * 4, true);
  CALLOC(c->sample_noisy, 64 * 4, true); CALLOC(c->sample_parts, 64 * 32 * sizeof(SamplePartial), true);
  CALLOC(c->filter_top_k, 64 * 4, true); CALLOC(c->filter_top_p, 64 * 4, true); CALLOC(c->filter_choice, 64 * 4, true);
  CALLOC(c->score_seq, B * P * 4, true); CALLOC(c->score_bsup, 64 * 4, true); CALLOC(c->score_sup, 1024 * 4, true);
  CALLOC(c->score_bits, ((V + 31) / 32 + 2048) * 4, true);
  CALLOC(c->score_parts, 64 * 32 * sizeof(ScorePartial), true);
  { int r = alloc_staging(c); if (r != TW_OK) return bail(r); }   // (here: the device block of the scores keeps its place among the allocations)
  // ---- dtw workspace ----
  CALLOC(c->zbuf, B * Ha * P * T * 4, false);
  CALLOC(c->mat, B * P * T * 4, false);
  CALLOC(c->trace, B * (P + 1) * (T + 1), false);
  CALLOC(c->out_ts, B * (P + 1) * 4, false);
  CALLOC(c->n_cols, B * 4, true);
#undef CALLOC
#undef CHIP
  *out = c;
  return TW_OK;
}

// ---------------------------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------------------------
int tw_load_weight(tw_ctx* c, const char* name_c, const void* src, int32_t sdt, int32_t ndim, const int64_t* shape,
                   void* stream) {
  if (!c || !name_c || !src || !shape) return fail(c, TW_EINVAL, "tw_load_weight: null argument");
  if (c->shares_weights) return fail(c, TW_ESTATE, "tw_load_weight: this context shares another context's weights (tw_create_sibling)");
  if (sdt != TW_F32 && sdt != TW_BF16 && sdt != TW_F16) return fail(c, TW_EINVAL, "unsupported source dtype %d", sdt);
  TW_ON_DEVICE(c);
  hipStream_t st = pick_stream(c, stream);
  const std::string name(name_c);
  const int d = c->d, F = c->ffn;
  long long numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= shape[i];
  auto want = [&](std::initializer_list<long long> s) -> bool {
    if ((int)s.size() != ndim) return false;
    int i = 0;
    for (long long v : s) if (shape[i++] != v) return false;
    return true;
  };
  auto conv = [&](void* dst, float scale) -> int {
    HIPCHK(c, launch_convert(c->dtype, sdt, src, dst, numel, scale, st));
    c->loaded.insert(name);
    return TW_OK;
  };
  auto bad_shape = [&]() { return fail(c, TW_ENAME, "shape mismatch for %s", name_c); };

  if (name == "proj_out.weight") return TW_OK;  // tied to embed_tokens (HF:models/whisper/modeling_whisper.py:965)
  if (name == "model.encoder.conv1.weight") {
    if (!want({d, c->n_mels, 3})) return bad_shape();
    HIPCHK(c, launch_conv_weight_reorder(c->dtype, sdt, src, c->conv1_w, d, c->n_mels, c->C, st));
    c->loaded.insert(name);
    return TW_OK;
  }
  if (name == "model.encoder.conv2.weight") {
    if (!want({d, d, 3})) return bad_shape();
    HIPCHK(c, launch_conv_weight_reorder(c->dtype, sdt, src, c->conv2_w, d, d, d, st));
    c->loaded.insert(name);
    return TW_OK;
  }
  if (name == "model.encoder.conv1.bias") return want({d}) ? conv(c->conv1_b, 1.f) : bad_shape();
  if (name == "model.encoder.conv2.bias") return want({d}) ? conv(c->conv2_b, 1.f) : bad_shape();
  if (name == "model.encoder.embed_positions.weight") {
    if (ndim != 2 || shape[1] != d || shape[0] > 1500) return bad_shape();
    HIPCHK(c, launch_convert(TW_F32, sdt, src, c->enc_pos_raw, numel, 1.f, st));
    c->loaded.insert(name);
    c->enc_pos_rows = (int)shape[0];
    return TW_OK;
  }
  if (name == "model.encoder.layer_norm.weight") return want({d}) ? conv(c->enc_ln_g, 1.f) : bad_shape();
  if (name == "model.encoder.layer_norm.bias") return want({d}) ? conv(c->enc_ln_b, 1.f) : bad_shape();
  if (name == "model.decoder.embed_tokens.weight") return want({c->V, d}) ? conv(c->tok_emb, 1.f) : bad_shape();
  if (name == "model.decoder.embed_positions.weight") {
    if (ndim != 2 || shape[1] != d || shape[0] < c->P) return bad_shape();
    numel = (long long)c->P * d;
    return conv(c->dec_pos, 1.f);
  }
  if (name == "model.decoder.layer_norm.weight") return want({d}) ? conv(c->dec_ln_g, 1.f) : bad_shape();
  if (name == "model.decoder.layer_norm.bias") return want({d}) ? conv(c->dec_ln_b, 1.f) : bad_shape();

  // per-layer tensors: model.{encoder|decoder}.layers.{i}.<rest>
  bool is_dec = false;
  size_t pos = std::string::npos;
  const std::string pe = "model.encoder.layers.", pd = "model.decoder.layers.";
  if (name.compare(0, pe.size(), pe) == 0) pos = pe.size();
  else if (name.compare(0, pd.size(), pd) == 0) { pos = pd.size(); is_dec = true; }
  if (pos == std::string::npos) return fail(c, TW_ENAME, "unknown weight name %s", name_c);
  const size_t dot = name.find('.', pos);
  if (dot == std::string::npos) return fail(c, TW_ENAME, "unknown weight name %s", name_c);
  const int li = std::atoi(name.substr(pos, dot - pos).c_str());
  const std::string rest = name.substr(dot + 1);
  std::vector<LayerW>& Ls = is_dec ? c->dec : c->enc;
  if (li < 0 || li >= (int)Ls.size()) return fail(c, TW_ENAME, "layer index out of range in %s", name_c);
  LayerW& L = Ls[li];
  const size_t e = c->esz;
  const float qs = 0.125f;  // head_dim^-0.5 for head_dim 64, exact in bf16: folded into q_proj (HF scales q before QK^T, :309)
  const bool isw = want({d, d}), isb = want({d});
  if (rest == "self_attn_layer_norm.weight") return isb ? conv(L.ln1_g, 1.f) : bad_shape();
  if (rest == "self_attn_layer_norm.bias") return isb ? conv(L.ln1_b, 1.f) : bad_shape();
  if (rest == "final_layer_norm.weight") return isb ? conv(L.ln2_g, 1.f) : bad_shape();
  if (rest == "final_layer_norm.bias") return isb ? conv(L.ln2_b, 1.f) : bad_shape();
  if (rest == "self_attn.q_proj.weight") return isw ? conv(L.wqkv, qs) : bad_shape();
  if (rest == "self_attn.q_proj.bias") return isb ? conv(L.bqkv, qs) : bad_shape();
  if (rest == "self_attn.k_proj.weight") return isw ? conv(at(L.wqkv, (size_t)d * d, e), 1.f) : bad_shape();
  if (rest == "self_attn.v_proj.weight") return isw ? conv(at(L.wqkv, (size_t)2 * d * d, e), 1.f) : bad_shape();
  if (rest == "self_attn.v_proj.bias") return isb ? conv(at(L.bqkv, (size_t)2 * d, e), 1.f) : bad_shape();
  if (rest == "self_attn.out_proj.weight") return isw ? conv(L.wo, 1.f) : bad_shape();
  if (rest == "self_attn.out_proj.bias") return isb ? conv(L.bo, 1.f) : bad_shape();
  if (rest == "fc1.weight") return want({F, d}) ? conv(L.w1, 1.f) : bad_shape();
  if (rest == "fc1.bias") return want({F}) ? conv(L.b1, 1.f) : bad_shape();
  if (rest == "fc2.weight") return want({d, F}) ? conv(L.w2, 1.f) : bad_shape();
  if (rest == "fc2.bias") return isb ? conv(L.b2, 1.f) : bad_shape();
  if (is_dec) {
    if (rest == "encoder_attn_layer_norm.weight") return isb ? conv(L.lnx_g, 1.f) : bad_shape();
    if (rest == "encoder_attn_layer_norm.bias") return isb ? conv(L.lnx_b, 1.f) : bad_shape();
    if (rest == "encoder_attn.q_proj.weight") return isw ? conv(L.wq_c, qs) : bad_shape();
    if (rest == "encoder_attn.q_proj.bias") return isb ? conv(L.bq_c, qs) : bad_shape();
    if (rest == "encoder_attn.k_proj.weight") return isw ? conv(L.wkv_c, 1.f) : bad_shape();
    if (rest == "encoder_attn.v_proj.weight") return isw ? conv(at(L.wkv_c, (size_t)d * d, e), 1.f) : bad_shape();
    if (rest == "encoder_attn.v_proj.bias") return isb ? conv(at(L.bkv_c, (size_t)d, e), 1.f) : bad_shape();
    if (rest == "encoder_attn.out_proj.weight") return isw ? conv(L.wo_c, 1.f) : bad_shape();
    if (rest == "encoder_attn.out_proj.bias") return isb ? conv(L.bo_c, 1.f) : bad_shape();
  }
  return fail(c, TW_ENAME, "unknown weight name %s", name_c);
}

int tw_finalize_weights(tw_ctx* c, void* stream) {
  if (!c) return TW_EINVAL;
  if (c->shares_weights) return fail(c, TW_ESTATE, "tw_finalize_weights: this context shares another context's weights (tw_create_sibling)");
  TW_ON_DEVICE(c);
  hipStream_t st = pick_stream(c, stream);
  const size_t expect = 4 + 1 + 2 + (size_t)c->Le * 15 + 2 + 2 + (size_t)c->Ld * 24;
  if (c->loaded.size() != expect) {
    return fail(c, TW_ESTATE, "tw_finalize_weights: %zu of %zu tensors loaded", c->loaded.size(), expect);
  }
  const int n_old = c->enc_pos_rows;  // rows of the positional table as loaded
  if (c->T > n_old) return fail(c, TW_EINVAL, "source_positions %d exceeds the positional table (%d rows)", c->T, n_old);
  // A0: patch_hf_model (R:thestage_speechkit/nvidia/asr_pipeline.py:15-27)
  HIPCHK(c, launch_interp_positions(c->dtype, TW_F32, c->enc_pos_raw, c->enc_pos, n_old, c->T, c->d, st));
  if (c->finalized) return fail(c, TW_ESTATE, "tw_finalize_weights called twice");
  // fold every decoder pre-LayerNorm into the projection that consumes it (k_decode.hip): W <- W*g, gw, cb
  for (int l = 0; l < c->Ld; ++l) {
    LayerW& L = c->dec[l];
    HIPCHK(c, launch_fold_ln(c->dtype, L.wqkv, L.wqkv, L.ln1_g, L.ln1_b, L.bqkv, L.qkv_gw, L.qkv_cb, 3 * c->d, c->d, st));
    HIPCHK(c, launch_fold_ln(c->dtype, L.wq_c, L.wq_c, L.lnx_g, L.lnx_b, L.bq_c, L.qc_gw, L.qc_cb, c->d, c->d, st));
    HIPCHK(c, launch_fold_ln(c->dtype, L.w1, L.w1, L.ln2_g, L.ln2_b, L.b1, L.fc1_gw, L.fc1_cb, c->ffn, c->d, st));
    if (c->fuse_cq) {
      // cross query ahead.  With x1 = x0 + attn Wo^T + bo (self-attention block) and W' the folded cross-query weight,
      //   x1 W'^T = x0 W'^T + attn (W' Wo)^T + W' bo:
      // rows [3d,4d) of the QKV matrix = W' (same operand x0 as q|k|v; ln_cb carries c0 = W' bo, no LayerNorm of ITS input),
      // rows [d,2d) of the out-projection = W' Wo (same operand attn).  The LayerNorm of x1 is applied by the consumer.
      const size_t dd = (size_t)c->d * c->d;
      HIPCHK(c, hipMemcpyAsync(at(L.wqkv, 3 * dd, c->esz), L.wq_c, dd * c->esz, hipMemcpyDeviceToDevice, st));
      HIPCHK(c, launch_compose(c->dtype, L.wq_c, L.wo, L.bo, at(L.wo, dd, c->esz), L.qkv_cb + 3 * c->d, c->d, c->d, c->d, st));
    }
  }
  HIPCHK(c, launch_fold_ln(c->dtype, c->logit_w, c->tok_emb, c->dec_ln_g, c->dec_ln_b, nullptr, c->logit_gw, c->logit_cb,
                           c->V, c->d, st));
  // ... and the encoder's two per layer into its QKV / fc1 GEMMs (k_gemm.hip, GemmEpilogue::stats_in): same algebra, the row
  // statistics come from the GEMM that wrote the residual stream
  for (int l = 0; l < c->Le && c->enc_fold; ++l) {
    LayerW& L = c->enc[l];
    HIPCHK(c, launch_fold_ln(c->dtype, L.wqkv, L.wqkv, L.ln1_g, L.ln1_b, L.bqkv, L.qkv_gw, L.qkv_cb, 3 * c->d, c->d, st));
    HIPCHK(c, launch_fold_ln(c->dtype, L.w1, L.w1, L.ln2_g, L.ln2_b, L.b1, L.fc1_gw, L.fc1_cb, c->ffn, c->d, st));
  }
  // decoder projections are consumed by launch_gemv in the fragment-major layout (k_decode.hip: tile_weights_kernel)
  {
    const size_t e = c->esz;
    const size_t Vp = (size_t)(c->V + 15) / 16 * 16;
    size_t mx = Vp * c->d;
    if ((size_t)4 * c->d * c->d > mx) mx = (size_t)4 * c->d * c->d;
    if ((size_t)c->ffn * c->d > mx) mx = (size_t)c->ffn * c->d;
    if ((size_t)3 * c->C * c->d > mx) mx = (size_t)3 * c->C * c->d;
    void* scratch = nullptr;
    HIPCHK(c, hipMalloc(&scratch, mx * e));
    // narrow projections (N <= 2048: the three d x d matrices and fc2) are laid out for 8-row tiles so that their launches
    // cover 160 instead of 80 compute units (k_decode.hip)
    auto retile = [&](void* w, int N, int K, unsigned char** scales, int* tr_out) -> int {
      const size_t Np = (size_t)(N + 15) / 16 * 16;
      const int tr = tr_out && N <= 2048 && N % 16 == 0 ? 8 : 16;
      if (tr_out) *tr_out = tr;
      if (c->w8) {  // MXFP8 fragments + block scales replace the bf16 rows in the same buffer (half the bytes + 1/32)
        unsigned char* sc = reinterpret_cast<unsigned char*>(scratch);
        HIPCHK(c, launch_quant_mx8(w, sc, sc + Np * K, N, K, tr, st));
        HIPCHK(c, hipMemcpyAsync(w, scratch, Np * K + Np * K / 32, hipMemcpyDeviceToDevice, st));
        *scales = reinterpret_cast<unsigned char*>(w) + Np * K;
      } else {
        HIPCHK(c, launch_tile_weights(c->dtype, w, scratch, N, K, tr, st));
        HIPCHK(c, hipMemcpyAsync(w, scratch, Np * K * e, hipMemcpyDeviceToDevice, st));
        *scales = nullptr;
      }
      return TW_OK;
    };
    int r = TW_OK;
    for (int l = 0; l < c->Ld && r == TW_OK; ++l) {
      LayerW& L = c->dec[l];
      // (both layouts are tile-major, so the unfused launches simply read the leading 3d / d rows of the fused buffers)
      if ((r = retile(L.wqkv, (c->fuse_cq ? 4 : 3) * c->d, c->d, &L.s_qkv, nullptr)) != TW_OK) break;   // K/V scatter epilogue: 16-row tiles
      // (the fused out-projection of large-v3 has 2560 rows: 16-row tiles = 160 workgroups, measured 1.487 vs 1.510 ms per step
      //  with 320 workgroups of 8 rows, each of which re-reads the whole activation block)
      if ((r = retile(L.wo, (c->fuse_cq ? 2 : 1) * c->d, c->d, &L.s_o, &L.tr_o)) != TW_OK) break;
      if ((r = retile(L.wq_c, c->d, c->d, &L.s_qc, &L.tr_qc)) != TW_OK) break;
      if ((r = retile(L.wo_c, c->d, c->d, &L.s_oc, &L.tr_oc)) != TW_OK) break;
      if ((r = retile(L.w1, c->ffn, c->d, &L.s_1, &L.tr_1)) != TW_OK) break;
      if ((r = retile(L.w2, c->d, c->ffn, &L.s_2, &L.tr_2)) != TW_OK) break;
    }
    if (r == TW_OK) r = retile(c->logit_w, c->V, c->d, &c->logit_ws, nullptr);
    // the MFMA GEMMs (k_gemm.hip) read their weight operand fragment-major too (16-row tiles, never quantised): encoder
    // projections, the conv stem as GEMMs over [co][3*C] / [co][3*d] rows, and the decoder's cross K|V projection
    auto retile_gemm = [&](void* w, int N, int K) -> int {
      HIPCHK(c, launch_tile_weights(c->dtype, w, scratch, N, K, 16, st));
      HIPCHK(c, hipMemcpyAsync(w, scratch, (size_t)N * K * e, hipMemcpyDeviceToDevice, st));
      return TW_OK;
    };
    if (r == TW_OK) r = retile_gemm(c->conv1_w, c->d, 3 * c->C);
    if (r == TW_OK) r = retile_gemm(c->conv2_w, c->d, 3 * c->d);
    for (int l = 0; l < c->Le && r == TW_OK; ++l) {
      LayerW& L = c->enc[l];
      if ((r = retile_gemm(L.wqkv, 3 * c->d, c->d)) != TW_OK) break;
      if ((r = retile_gemm(L.wo, c->d, c->d)) != TW_OK) break;
      if ((r = retile_gemm(L.w1, c->ffn, c->d)) != TW_OK) break;
      if ((r = retile_gemm(L.w2, c->d, c->ffn)) != TW_OK) break;
    }
    for (int l = 0; l < c->Ld && r == TW_OK; ++l) r = retile_gemm(c->dec[l].wkv_c, 2 * c->d, c->d);
    hipError_t he = hipStreamSynchronize(st);
    hipFree(scratch);
    if (r != TW_OK) return r;
    HIPCHK(c, he);
  }
  c->finalized = true;
  return TW_OK;
}

// ---------------------------------------------------------------------------------------------
// A1 log-mel
// ---------------------------------------------------------------------------------------------
int tw_logmel(tw_ctx* c, const float* pcm, int64_t pcm_stride, const int32_t* n_valid_host, int32_t B, int32_t n_samples,
              void* out, int32_t out_dtype, void* stream) {
  if (!c || !pcm || !out) return fail(c, TW_EINVAL, "tw_logmel: null argument");
  TW_ON_DEVICE(c);
  if (B < 1 || B > c->Bmax) return fail(c, TW_EINVAL, "tw_logmel: B=%d outside [1,%d]", B, c->Bmax);
  if (n_samples < 400 || n_samples % 160 != 0) return fail(c, TW_EINVAL, "n_samples must be a multiple of 160 and >= 400");
  if ((size_t)B * c->n_mels * (n_samples / 160) > c->logspec_cap)
    return fail(c, TW_EINVAL, "tw_logmel: n_samples=%d exceeds the context capacity (%d frames)", n_samples, 2 * c->T);
  if (out_dtype != TW_F32 && out_dtype != c->dtype) return fail(c, TW_EINVAL, "out_dtype must be TW_F32 or the context dtype");
  hipStream_t st = pick_stream(c, stream);
  const int* nv = nullptr;
  if (n_valid_host) {
    memcpy(c->h_pinned->n_valid, n_valid_host, sizeof(int) * B);
    HIPCHK(c, hipMemcpyAsync(c->n_valid_dev, c->h_pinned->n_valid, sizeof(int) * B, hipMemcpyHostToDevice, st));
    nv = c->n_valid_dev;
  }
  tic(c, 0, st);
  HIPCHK(c, launch_logmel(pcm, pcm_stride, nv, B, n_samples, c->n_mels, c->lm, c->logspec_ws, c->lm_max, out, out_dtype, st));
  toc(c, 0, st);
  if (n_valid_host) HIPCHK(c, hipStreamSynchronize(st));  // pinned staging buffer is reused
  return TW_OK;
}

// ---------------------------------------------------------------------------------------------
// A2-A4 encoder
// ---------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// encoder for B clips whose output goes to slots slot0 .. slot0+B-1 of enc_out (all other buffers are scratch from row 0)
// `taps` (tw_encode_tapped, a test instrument): copies of whole workspace buffers right after the launch that wrote them; null on
// every product path, where each tap below is one untaken branch
int encode_core(tw_ctx* c, const void* mel, int32_t mel_dtype, int32_t B, int32_t slot0, void* out_hidden, int32_t out_dtype,
                void* stream, const tw_encode_taps* taps = nullptr) {
  if (!c || !mel) return fail(c, TW_EINVAL, "tw_encode: null argument");
  TW_ON_DEVICE(c);
  if (!c->finalized) return fail(c, TW_ESTATE, "tw_encode before tw_finalize_weights");
  if (B < 1 || slot0 < 0 || slot0 + B > c->Bmax) return fail(c, TW_EINVAL, "tw_encode: slots [%d, %d) outside [0,%d)", slot0, slot0 + B, c->Bmax);
  if (slot0 > c->encoded_B) return fail(c, TW_ESTATE, "tw_encode_at: slot0=%d but only %d slots are filled", slot0, c->encoded_B);
  if (mel_dtype != TW_F32 && mel_dtype != TW_BF16 && mel_dtype != TW_F16) return fail(c, TW_EINVAL, "tw_encode: mel_dtype %d is not TW_F32 / TW_BF16 / TW_F16", mel_dtype);
  if (out_hidden && out_dtype != TW_F32 && out_dtype != TW_BF16 && out_dtype != TW_F16)
    return fail(c, TW_EINVAL, "tw_encode: out_dtype %d is not TW_F32 / TW_BF16 / TW_F16", out_dtype);
  hipStream_t st = pick_stream(c, stream);
  const int d = c->d, T = c->T, C = c->C, H = c->H, F = c->ffn, dt = c->dtype;
  const size_t e = c->esz;
  const bool fold = c->enc_fold;
  if (taps && (taps->layer < 0 || taps->layer >= c->Le)) return fail(c, TW_EINVAL, "tw_encode_tapped: layer %d outside [0,%d)", taps->layer, c->Le);
  if (taps && !fold && (taps->ln_stats_a || taps->ln_stats_b)) return fail(c, TW_EINVAL, "tw_encode_tapped: this context keeps no LayerNorm statistics");
  const size_t rows_max = (size_t)c->Bmax * T;   // the workspace is sized for Bmax clips and a tap takes all of it
  auto tap = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
  };
  tic(c, 1, st);
  HIPCHK(c, launch_mel_transpose(dt, mel_dtype, mel, c->melT, B, c->n_mels, 2 * T, C, st));
  {  // conv1 (k3,p1) + GELU as a GEMM over overlapping 3-row windows of the padded token-major mel
    GemmEpilogue ep{};
    ep.bias = c->conv1_b; ep.gelu = 1; ep.mode = EPI_ROWMAJOR;
    ep.c_map = RowMap{2 * T, (long long)(2 * T + 2) * d, d};
    ep.out = at(c->h1, d, e);
    HIPCHK(c, launch_gemm(dt, c->melT, RowMap{2 * T, (long long)(2 * T + 2) * C, C}, c->conv1_w, B * 2 * T, d, 3 * C, ep, st));
    if (taps) HIPCHK(c, tap(taps->h1, c->h1, (size_t)c->Bmax * (2 * T + 2) * d * e));
  }
  {  // conv2 (k3,s2,p1) + GELU + positions: windows of 3 rows at stride 2 rows
    GemmEpilogue ep{};
    ep.bias = c->conv2_b; ep.gelu = 1; ep.mode = EPI_ROWMAJOR;
    ep.res = c->enc_pos; ep.res_map = plain_rows(d); ep.res_mod = T;
    ep.c_map = plain_rows(d);
    ep.out = c->xa;
    if (fold) ep.stats_out = c->ln_stats_a;
    HIPCHK(c, launch_gemm(dt, c->h1, RowMap{T, (long long)(2 * T + 2) * d, 2LL * d}, c->conv2_w, B * T, d, 3 * d, ep, st));
  }
  const int M = B * T;
  for (int l = 0; l < c->Le; ++l) {
    const LayerW& L = c->enc[l];
    const tw_encode_taps* tp = taps && taps->layer == l ? taps : nullptr;
    if (tp) {   // the layer's input: what conv2 (l = 0) or the fc2 of layer l - 1 left
      HIPCHK(c, tap(tp->xa_in, c->xa, rows_max * d * e));
      HIPCHK(c, tap(tp->ln_stats_a, c->ln_stats_a, rows_max * (d / 32) * 8));
    }
    // pre-LayerNorms: folded into the consuming GEMM (weights carry the gain, the epilogue applies mean / rstd from the partial row
    // statistics the producing GEMM left), or - without enc_fold - a launch that writes a normalised copy
    if (!fold) HIPCHK(c, launch_layernorm(dt, c->xa, L.ln1_g, L.ln1_b, c->lnbuf, M, d, st));
    {
      GemmEpilogue ep{};
      ep.bias = L.bqkv; ep.mode = EPI_QKV_ENC; ep.T = T; ep.Tp = c->Tp; ep.H = H;
      ep.out = c->qbuf; ep.out2 = c->kbuf; ep.out3 = c->vtbuf;
      if (fold) { ep.bias = nullptr; ep.stats_in = c->ln_stats_a; ep.stats_in_parts = d / 32; ep.ln_gw = L.qkv_gw; ep.ln_cb = L.qkv_cb; }
      HIPCHK(c, launch_gemm(dt, fold ? c->xa : c->lnbuf, plain_rows(d), L.wqkv, M, 3 * d, d, ep, st));
      if (tp) {
        HIPCHK(c, tap(tp->q, c->qbuf, rows_max * d * e));
        HIPCHK(c, tap(tp->k, c->kbuf, rows_max * d * e));
        HIPCHK(c, tap(tp->vt, c->vtbuf, (size_t)c->Bmax * H * 64 * c->Tp * e));
      }
    }
    HIPCHK(c, launch_enc_attention(dt, c->qbuf, c->kbuf, c->vtbuf, c->attn, B, H, T, c->Tp, st));
    if (tp) HIPCHK(c, tap(tp->attn, c->attn, rows_max * d * e));
    {
      GemmEpilogue ep{};
      ep.bias = L.bo; ep.mode = EPI_ROWMAJOR; ep.res = c->xa; ep.res_map = plain_rows(d); ep.c_map = plain_rows(d);
      ep.out = c->xb;
      if (fold) ep.stats_out = c->ln_stats_b;
      HIPCHK(c, launch_gemm(dt, c->attn, plain_rows(d), L.wo, M, d, d, ep, st));
      if (tp) {
        HIPCHK(c, tap(tp->xb, c->xb, rows_max * d * e));
        HIPCHK(c, tap(tp->ln_stats_b, c->ln_stats_b, rows_max * (d / 32) * 8));
      }
    }
    if (!fold) HIPCHK(c, launch_layernorm(dt, c->xb, L.ln2_g, L.ln2_b, c->lnbuf, M, d, st));
    {
      GemmEpilogue ep{};
      ep.bias = L.b1; ep.gelu = 1; ep.mode = EPI_ROWMAJOR; ep.c_map = plain_rows(F); ep.out = c->ffnh;
      if (fold) { ep.bias = nullptr; ep.stats_in = c->ln_stats_b; ep.stats_in_parts = d / 32; ep.ln_gw = L.fc1_gw; ep.ln_cb = L.fc1_cb; }
      HIPCHK(c, launch_gemm(dt, fold ? c->xb : c->lnbuf, plain_rows(d), L.w1, M, F, d, ep, st));
      if (tp) HIPCHK(c, tap(tp->ffnh, c->ffnh, rows_max * F * e));
    }
    {
      GemmEpilogue ep{};
      ep.bias = L.b2; ep.mode = EPI_ROWMAJOR; ep.res = c->xb; ep.res_map = plain_rows(d); ep.c_map = plain_rows(d);
      ep.out = c->xa;
      if (fold && l + 1 < c->Le) ep.stats_out = c->ln_stats_a;
      HIPCHK(c, launch_gemm(dt, c->ffnh, plain_rows(F), L.w2, M, d, F, ep, st));
      if (tp) HIPCHK(c, tap(tp->xa_out, c->xa, rows_max * d * e));
    }
  }
  void* enc_dst = at(c->enc_out, (size_t)slot0 * T * d, e);
  HIPCHK(c, launch_layernorm(dt, c->xa, c->enc_ln_g, c->enc_ln_b, enc_dst, M, d, st));
  if (taps) HIPCHK(c, tap(taps->enc_out, c->enc_out, rows_max * d * e));
  toc(c, 1, st);
  if (out_hidden) HIPCHK(c, launch_convert(out_dtype, dt, enc_dst, out_hidden, (long long)M * d, 1.f, st));
  c->encoded_B = slot0 + B;
  c->cross_B = slot0 < c->cross_B ? slot0 : c->cross_B;   // cross K/V of the re-encoded slots (and everything after) is stale
  return TW_OK;
}

// cross K/V of slots slot0 .. slot0+B-1: the per-(stream, head) blocks of a layer are contiguous per stream, so a slot offset is
// a pointer offset on the GEMM's input rows and on its head-split outputs
int cross_kv_core(tw_ctx* c, int32_t B, int32_t slot0, void* stream) {
  if (!c) return TW_EINVAL;
  TW_ON_DEVICE(c);
  if (B < 1 || slot0 < 0 || slot0 + B > c->encoded_B)
    return fail(c, TW_ESTATE, "tw_cross_kv: slots [%d, %d) but %d clips encoded", slot0, slot0 + B, c->encoded_B);
  if (slot0 > c->cross_B) return fail(c, TW_ESTATE, "tw_cross_kv_at: slot0=%d but cross K/V holds %d clips", slot0, c->cross_B);
  hipStream_t st = pick_stream(c, stream);
  const int d = c->d, T = c->T;
  const size_t per_layer = (size_t)c->Bmax * c->Tp * d;
  const size_t slot_off = (size_t)slot0 * c->Tp * d;             // elements of one layer's K (or V^T) arena before slot0
  const size_t sc_off = (size_t)slot0 * c->H * c->Tp;            // fp8 contexts: scale bytes before slot0
  tic(c, 2, st);
  for (int l = 0; l < c->Ld; ++l) {
    const LayerW& L = c->dec[l];
    GemmEpilogue ep{};
    ep.bias = L.bkv_c; ep.mode = c->w8 ? EPI_KV_CROSS8 : EPI_KV_CROSS; ep.T = T; ep.Tp = c->Tp; ep.H = c->H;
    ep.out = at(c->cross_k, per_layer * l + slot_off, c->w8 ? 1 : c->esz);
    ep.out2 = at(c->cross_v, per_layer * l + slot_off, c->w8 ? 1 : c->esz);
    if (c->w8) {
      ep.out3 = c->cross_ksc + (size_t)c->Bmax * c->H * c->Tp * l + sc_off;
      ep.out4 = c->cross_vsc + (size_t)c->Bmax * c->H * c->Tp * l + sc_off;
    }
    HIPCHK(c, launch_gemm(c->dtype, at(c->enc_out, (size_t)slot0 * T * d, c->esz), plain_rows(d), L.wkv_c, B * T, 2 * d, d, ep, st));
  }
  toc(c, 2, st);
  c->cross_B = slot0 + B;
  return TW_OK;
}

}  // namespace

extern "C" {

int tw_encode(tw_ctx* c, const void* mel, int32_t mel_dtype, int32_t B, void* out_hidden, int32_t out_dtype, void* stream) {
  if (c) { c->encoded_B = 0; c->cross_B = 0; }
  return encode_core(c, mel, mel_dtype, B, 0, out_hidden, out_dtype, stream);
}

int tw_encode_tapped(tw_ctx* c, const void* mel, int32_t mel_dtype, int32_t B, void* out_hidden, int32_t out_dtype,
                     const tw_encode_taps* taps, void* stream) {
  if (c) { c->encoded_B = 0; c->cross_B = 0; }
  return encode_core(c, mel, mel_dtype, B, 0, out_hidden, out_dtype, stream, taps);
}

int tw_gemm_plan(int32_t dtype, int32_t mode, int32_t M, int32_t N, int32_t K, int32_t* kernel, int32_t* bm) {
  if (dtype != TW_F32 && dtype != TW_BF16 && dtype != TW_F16) return fail(nullptr, TW_EINVAL, "tw_gemm_plan: dtype %d is not TW_F32 / TW_BF16 / TW_F16", dtype);
  if (mode != EPI_ROWMAJOR && mode != EPI_QKV_ENC && mode != EPI_KV_CROSS) return fail(nullptr, TW_EINVAL, "tw_gemm_plan: mode %d", mode);
  const int kt = dtype == TW_F32 ? 32 : 64;   // elements per K tile (k_gemm.hip)
  if (M < 1 || N < 64 || N % 64 != 0 || K < kt || K % kt != 0) return fail(nullptr, TW_EINVAL, "tw_gemm_plan: no GEMM for M=%d N=%d K=%d", M, N, K);
  const GemmPlan p = gemm_plan(mode, M, N);
  if (kernel) *kernel = p.kernel;
  if (bm) *bm = p.bm;
  return TW_OK;
}

int tw_enc_attention_plan(int32_t dtype, int32_t B, int32_t H, int32_t T, int32_t* queries_per_block, int32_t* xcd) {
  if (dtype != TW_F32 && dtype != TW_BF16 && dtype != TW_F16) return fail(nullptr, TW_EINVAL, "tw_enc_attention_plan: dtype %d is not TW_F32 / TW_BF16 / TW_F16", dtype);
  if (B < 1 || H < 1 || T < 1) return fail(nullptr, TW_EINVAL, "tw_enc_attention_plan: B=%d H=%d T=%d", B, H, T);
  const EncAttnPlan p = enc_attention_plan(dtype, B, H, T);
  if (queries_per_block) *queries_per_block = p.queries_per_block;
  if (xcd) *xcd = p.xcd;
  return TW_OK;
}

int tw_encode_at(tw_ctx* c, const void* mel, int32_t mel_dtype, int32_t B, int32_t slot0, void* stream) {
  if (c && slot0 == 0) { c->encoded_B = 0; c->cross_B = 0; }
  return encode_core(c, mel, mel_dtype, B, slot0, nullptr, 0, stream);
}

int tw_cross_kv(tw_ctx* c, int32_t B, void* stream) {
  if (c) c->cross_B = 0;
  return cross_kv_core(c, B, 0, stream);
}

int tw_cross_kv_at(tw_ctx* c, int32_t B, int32_t slot0, void* stream) { return cross_kv_core(c, B, slot0, stream); }

int tw_adopt_cross_kv(tw_ctx* dst, int32_t dst_slot0, tw_ctx* src, int32_t src_slot0, int32_t B, void* stream, void* src_stream) {
  if (!dst || !src) return fail(dst, TW_EINVAL, "tw_adopt_cross_kv: null context");
  TW_ON_DEVICE(dst);
  if (dst == src) return fail(dst, TW_EINVAL, "tw_adopt_cross_kv: source and destination are the same context");
  if (dst->cfg.device != src->cfg.device || dst->d != src->d || dst->H != src->H || dst->Ld != src->Ld || dst->T != src->T ||
      dst->Tp != src->Tp || dst->dtype != src->dtype || dst->w8 != src->w8)
    return fail(dst, TW_EINVAL, "tw_adopt_cross_kv: the contexts differ (model dimensions, source_positions, dtype or device)");
  if (B < 1 || src_slot0 < 0 || src_slot0 + B > src->cross_B)
    return fail(dst, TW_ESTATE, "tw_adopt_cross_kv: source slots [%d, %d) but the source holds cross K/V of %d clips", src_slot0, src_slot0 + B, src->cross_B);
  if (dst_slot0 < 0 || dst_slot0 + B > dst->Bmax) return fail(dst, TW_EINVAL, "tw_adopt_cross_kv: destination slots [%d, %d) outside [0,%d)", dst_slot0, dst_slot0 + B, dst->Bmax);
  if (dst_slot0 > dst->cross_B) return fail(dst, TW_ESTATE, "tw_adopt_cross_kv: dst_slot0=%d but the destination holds %d clips", dst_slot0, dst->cross_B);
  hipStream_t st = pick_stream(dst, stream);
  hipStream_t sst = pick_stream(src, src_stream);
  // the copies follow everything `src` has enqueued so far (its encoder + cross-K/V launches) ...
  if (sst != st) {
    HIPCHK(dst, hipEventRecord(dst->ring_ev[0], sst));
    HIPCHK(dst, hipStreamWaitEvent(st, dst->ring_ev[0], 0));
  }
  // one 2-D copy per arena: row l = layer l, `width` bytes of B consecutive slots, pitches = one layer of each context
  const size_t slot_bytes = (size_t)dst->Tp * dst->d * (dst->w8 ? 1 : dst->esz);
  auto copy = [&](void* d_base, const void* s_base, size_t per_slot) -> hipError_t {
    return hipMemcpy2DAsync(reinterpret_cast<char*>(d_base) + (size_t)dst_slot0 * per_slot, (size_t)dst->Bmax * per_slot,
                            reinterpret_cast<const char*>(s_base) + (size_t)src_slot0 * per_slot, (size_t)src->Bmax * per_slot,
                            (size_t)B * per_slot, (size_t)dst->Ld, hipMemcpyDeviceToDevice, st);
  };
  HIPCHK(dst, copy(dst->cross_k, src->cross_k, slot_bytes));
  HIPCHK(dst, copy(dst->cross_v, src->cross_v, slot_bytes));
  if (dst->w8) {
    const size_t sc = (size_t)dst->H * dst->Tp;
    HIPCHK(dst, copy(dst->cross_ksc, src->cross_ksc, sc));
    HIPCHK(dst, copy(dst->cross_vsc, src->cross_vsc, sc));
  }
  // ... and whatever `src` enqueues next (it may refill these slots) follows the copies
  if (sst != st) {
    HIPCHK(dst, hipEventRecord(dst->ring_ev[1], st));
    HIPCHK(dst, hipStreamWaitEvent(sst, dst->ring_ev[1], 0));
  }
  dst->cross_B = dst_slot0 + B;
  if (dst->encoded_B < dst->cross_B) dst->encoded_B = dst->cross_B;   // (the encoder states themselves stay in `src`: nothing reads them after A5)
  return TW_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------------------------
namespace {

// TW_FUSE_CQ=0 at run time: the unfused launch sequence on the same (fused-layout) weights, for A/B measurements
bool getenv_off_fuse() {
  static const bool off = []() { const char* e = getenv("TW_FUSE_CQ"); return e && atoi(e) == 0; }();
  return off;
}

// What one decode_core pass is asked for.  The defaults are tw_decode_step's pass; every other caller names what differs.
struct DecodeOpts {
  // > 0: rows mode (tw_common.h: tw_row_of) - the B rows are rows_streams streams x B / rows_streams consecutive positions whose
  // tokens are `ids` (device, row order)
  int rows_streams = 0;
  const int* ids = nullptr;
  // false: the input rows are already in place (the sampler's last launch of the previous step wrote them, SamplerArgs::x_next)
  bool embed = true;
  // the tied-logits projection of every row.  false: the tokens of the rows' positions are known (prefill_core).  Rows mode with it
  // (draft-and-verify: verify_round) is the same launch the step uses, so a row's logits are bit for bit what the one-position step
  // would have produced (k_decode.hip: one reduction order for every B)
  bool logits = true;
  // false: the cross attention is launched with Ha = 0 and no slot table, so the alignment rows an earlier tw_generate_greedy
  // recorded stay as they are (tw_score_tokens); its output does not depend on it
  bool record_alignment = true;
  // != nullptr (device, [64]): a step of tw_generate_greedy_ragged (ordinary step only) - the embedding (the step's own, whatever
  // `embed` says), the K / V^T scatter of the QKV launch and the self attention are the ragged instantiations (tw_common.h:
  // tw_row_pos); every other launch is the plain step's
  const int* n_pad = nullptr;
};

// one token for every stream: embed -> Ld layers -> final LN + tied logits (fp32)
int decode_core(tw_ctx* c, int B, hipStream_t st, const DecodeOpts& o = DecodeOpts{}) {
  const int d = c->d, H = c->H, F = c->ffn, T = c->T, P = c->P, dt = c->dtype;
  const size_t e = c->esz;
  const int rs = o.rows_streams; const int* n_pad = o.n_pad;
  if (n_pad && rs != 0) return fail(c, TW_EINVAL, "decode_core: a ragged step is an ordinary step with its own embedding");
  if (n_pad) HIPCHK(c, launch_embed_ragged(dt, c->cur_ids, c->stt, n_pad, c->tok_emb, c->dec_pos, c->dx0, B, d, st));
  else if (o.embed) HIPCHK(c, launch_embed(dt, rs > 0 ? o.ids : c->cur_ids, c->stt, c->tok_emb, c->dec_pos, c->dx0, B, d, rs, st));
  void* xin = c->dx0;
  void* xmid = c->dx1;
  const int Pp = (P + 63) / 64 * 64;
  const size_t self_layer = (size_t)c->Bmax * Pp * d;
  const size_t cross_layer = (size_t)c->Bmax * c->Tp * d;
  for (int l = 0; l < c->Ld; ++l) {
    const LayerW& L = c->dec[l];
    void* sk = at(c->self_k, self_layer * l, e);
    void* sv = at(c->self_v, self_layer * l, e);
    // "cross query ahead" (tw_ctx::fuse_cq): the cross-attention query u = x1 . W'^T is accumulated by the two projections
    // before it - x0 . W'^T as a fourth segment of the QKV launch, attn . (W' Wo)^T as a second half of the out-projection
    // launch - and the cross attention applies the folded LayerNorm of x1 itself: 7 instead of 8 dependent launches per layer
    const bool fq_on = c->fuse_cq && !getenv_off_fuse() && d / (L.tr_o ? L.tr_o : 16) <= 192;
    {  // LN + fused QKV; k,v rows go straight into the cache at position pos
      GemvArgs a{};
      a.x = xin; a.ldx = d; a.ln_gw = L.qkv_gw; a.ln_cb = L.qkv_cb; a.W = L.wqkv; a.wscale = L.s_qkv; a.a16 = c->a16; a.N = (fq_on ? 4 : 3) * d; a.K = d; a.B = B;
      a.y = c->dq; a.ldy = d; a.kcache = sk; a.vcache = sv; a.cache_bstride = (long long)Pp * d; a.cache_hstride = (long long)Pp * 64; a.d_model = d; a.stt = c->stt;
      a.u = fq_on ? c->du : nullptr;
      a.rows_streams = rs;
      a.n_pad = n_pad;
      HIPCHK(c, launch_gemv(dt, a, st));
    }
    if (n_pad) HIPCHK(c, launch_dec_self_attn_ragged(dt, c->dq, sk, sv, Pp, c->datt, B, H, c->dec_key_bound > 0 ? c->dec_key_bound : P, c->stt, n_pad, st));
    else HIPCHK(c, launch_dec_self_attn(dt, c->dq, sk, sv, Pp, c->datt, B, H, c->dec_key_bound > 0 ? c->dec_key_bound : P, c->stt, rs, st));
    {
      GemvArgs a{};
      a.x = c->datt; a.ldx = d; a.W = L.wo; a.wscale = L.s_o; a.a16 = c->a16; a.tr = L.tr_o; a.bias = L.bo; a.N = (fq_on ? 2 : 1) * d; a.K = d; a.B = B;
      a.res = xin; a.ldres = d; a.y = xmid; a.ldy = d;
      if (fq_on) { a.u = c->du; a.nsplit = d; a.stats = c->dstats; }
      HIPCHK(c, launch_gemv(dt, a, st));
    }
    FusedQ fq{};
    if (fq_on) {
      fq.u = c->du; fq.stats = c->dstats; fq.n_part = d / (L.tr_o ? L.tr_o : 16); fq.gw = L.qc_gw; fq.cb = L.qc_cb; fq.d = d;
    } else {
      GemvArgs a{};
      a.x = xmid; a.ldx = d; a.ln_gw = L.qc_gw; a.ln_cb = L.qc_cb; a.W = L.wq_c; a.wscale = L.s_qc; a.a16 = c->a16; a.tr = L.tr_qc; a.N = d; a.K = d; a.B = B;
      a.y = c->dq; a.ldy = d;
      HIPCHK(c, launch_gemv(dt, a, st));
    }
    HIPCHK(c, launch_dec_cross_attn(dt, c->dq, fq, at(c->cross_k, cross_layer * l, c->w8 ? 1 : e), at(c->cross_v, cross_layer * l, c->w8 ? 1 : e),
                                    c->datt, B, H, T, c->Tp, (c->Ha > 0 && o.record_alignment) ? c->align_slot + (size_t)l * H : nullptr, c->align,
                                    o.record_alignment ? c->Ha : 0,
                                    P, c->stt, c->w8 ? c->cross_ksc + (size_t)c->Bmax * H * c->Tp * l : nullptr,
                                    c->w8 ? c->cross_vsc + (size_t)c->Bmax * H * c->Tp * l : nullptr, rs, st));
    {
      GemvArgs a{};
      a.x = c->datt; a.ldx = d; a.W = L.wo_c; a.wscale = L.s_oc; a.a16 = c->a16; a.tr = L.tr_oc; a.bias = L.bo_c; a.N = d; a.K = d; a.B = B; a.res = xmid; a.ldres = d;
      a.y = xin; a.ldy = d;
      HIPCHK(c, launch_gemv(dt, a, st));
    }
    {
      GemvArgs a{};
      a.x = xin; a.ldx = d; a.ln_gw = L.fc1_gw; a.ln_cb = L.fc1_cb; a.W = L.w1; a.wscale = L.s_1; a.a16 = c->a16; a.tr = L.tr_1; a.N = F; a.K = d; a.B = B;
      a.gelu = 1; a.y = c->dh; a.ldy = F;
      HIPCHK(c, launch_gemv(dt, a, st));
    }
    {
      GemvArgs a{};
      a.x = c->dh; a.ldx = F; a.W = L.w2; a.wscale = L.s_2; a.a16 = c->a16; a.tr = L.tr_2; a.bias = L.b2; a.N = d; a.K = F; a.B = B; a.res = xin; a.ldres = d;
      a.y = xmid; a.ldy = d;
      HIPCHK(c, launch_gemv(dt, a, st));
    }
    void* t = xin; xin = xmid; xmid = t;
  }
  if (o.logits) {
    GemvArgs a{};
    a.x = xin; a.ldx = d; a.ln_gw = c->logit_gw; a.ln_cb = c->logit_cb; a.W = c->logit_w; a.wscale = c->logit_ws; a.a16 = c->a16; a.N = c->V; a.K = d; a.B = B;
    a.y_f32 = c->logits;
    HIPCHK(c, launch_gemv(dt, a, st));
  }
  return TW_OK;
}

// rows of a rows-mode launch (B streams x consecutive positions): W8A8 quantises activations per group of 16 rows, one group per launch
int rows_per_launch(const tw_ctx* c) { return (c->w8 && !c->a16) ? 16 : 64; }

// dec_key_bound of a launch whose last position is n_keys - 1: the self attention reads keys [0, n_keys) in whole 64-key buckets, and
// never past the bucket of `limit` (the cache's P, or a call's max_len)
int key_bound(int n_keys, int limit) { return std::min((n_keys + 63) / 64 * 64, (limit + 63) / 64 * 64); }

// The position-major row tables of a rows-mode pass over positions [p_first, p_last] of B streams whose tokens are tok[b * ld + p]: row
// (p - p_first) * B + b (row r of the launch at p0 is stream r % B at position p0 + r / B) holds, in h_rows.tok, the token at p and -
// with_lastts - in h_rows.lastts the last timestamp token (>= ts_begin) among the sampled tokens (positions >= n_begin) up to p, or -1
void fill_row_tables(tw_ctx* c, int B, const int* tok, int ld, int p_first, int p_last, bool with_lastts, int n_begin, int ts_begin) {
  for (int b = 0; b < B; ++b) {
    int lt = -1;
    for (int p = with_lastts ? std::min(n_begin, p_first) : p_first; p <= p_last; ++p) {
      const int t = tok[(size_t)b * ld + p];
      if (p >= n_begin && t >= ts_begin) lt = t;
      if (p < p_first) continue;
      c->h_rows.tok[(size_t)(p - p_first) * B + b] = t;
      if (with_lastts) c->h_rows.lastts[(size_t)(p - p_first) * B + b] = lt;
    }
  }
}

// Batched prefill of the positions [0, n_pos) of B streams whose tokens are known (host table tok[b * ld + p]): launches of up to
// `cap` rows = B streams x L consecutive positions (rows mode), each a full pass through the decoder layers that fills the
// self-attention caches and the alignment rows of its positions; the weights are streamed once per L positions instead of once per
// position.  On return the device position is n_pos.  Not captured in a graph (a handful of launches per call).
int prefill_core(tw_ctx* c, int B, const int* tok, int ld, int n_pos, hipStream_t st) {
  if (n_pos <= 0) return TW_OK;
  const int cap = rows_per_launch(c);
  if (B > cap) return fail(c, TW_EINVAL, "prefill: %d streams exceed the %d rows of a launch", B, cap);
  const int L = std::max(1, cap / B);
  if ((size_t)n_pos * B > c->row_ids_cap) return fail(c, TW_EINVAL, "prefill: %d positions x %d streams exceed the row table", n_pos, B);
  fill_row_tables(c, B, tok, ld, 0, n_pos - 1, false, 0, 0);
  HIPCHK(c, hipMemcpyAsync(c->row_ids, c->h_rows.tok, sizeof(int) * (size_t)n_pos * B, hipMemcpyHostToDevice, st));
  DecodeOpts rows; rows.rows_streams = B; rows.logits = false;
  for (int p0 = 0; p0 < n_pos; p0 += L) {
    const int l = std::min(L, n_pos - p0);
    c->dec_key_bound = key_bound(p0 + l, c->P);
    rows.ids = c->row_ids + (size_t)p0 * B;
    int r = decode_core(c, l * B, st, rows);
    if (r != TW_OK) return r;
    HIPCHK(c, launch_advance(c->stt, l, st));
  }
  return TW_OK;
}

// One ROUND of draft-and-verify (tw_greedy_opts::n_draft).  tok[b * ld + p] holds, for every stream, the true tokens at
// positions <= p_start and GUESSES behind them; the device position is p_start.  Positions [p_start, p_end] are run in rows mode
// (launches of up to rows_cap rows = B streams x consecutive positions, each with the logits of every row and the sampler's choice for
// every row - the processors see the given tokens as history), and the round ends at the first position p_acc where some stream's
// choice differs from the token the next row was given (or at p_end): the choices at p_acc become the tokens at p_acc + 1 - exactly
// what the one-position loop would have produced there, because a row's logits do not depend on which other rows share its launch
// (k_decode.hip) and every earlier given token was confirmed - and the device state (history, last timestamp, finished flags,
// position) is the loop's state after that token.  The host synchronises once per launch (it needs the decision to go on).
// On return *p_next = p_acc + 1 and tok[.. + *p_next] holds those tokens.
// *next_given = 1 when the tokens the round PRODUCED at *p_next are (for every stream) the guesses that stood there (p_next <= p_given).
// ba != nullptr (tw_generate_greedy_biased): every launch's logits pass through launch_seq_bias before its sampler, rows mode.
// ra != nullptr (tw_generate_greedy_repeat): ... and through launch_repeat, behind the bias.
int verify_round(tw_ctx* c, int B, int* tok, int ld, int n_begin, int ts_begin, int p_start, int p_end, int rows_cap, const SamplerArgs& sa0,
                 hipStream_t st, int* p_next, int p_given, int* next_given, const SeqBiasArgs* ba, const RepeatArgs* ra) {
  const int n_pos = p_end - p_start + 1;
  if (n_pos < 1 || B > rows_cap) return fail(c, TW_EINVAL, "verify: bad round [%d, %d] for %d streams", p_start, p_end, B);
  if ((size_t)n_pos * B > c->row_ids_cap) return fail(c, TW_EINVAL, "verify: %d positions x %d streams exceed the row table", n_pos, B);
  const int L = std::max(1, rows_cap / B);
  fill_row_tables(c, B, tok, ld, p_start, p_end, true, n_begin, ts_begin);
  VerifyStage* hv = c->h_verify;
  hv->reset[0] = 0x7fffffff; hv->reset[1] = 0;   // no mismatch yet, undecided
  HIPCHK(c, hipMemcpyAsync(c->row_ids, c->h_rows.tok, sizeof(int) * (size_t)n_pos * B, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->row_lastts, c->h_rows.lastts, sizeof(int) * (size_t)n_pos * B, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->verify_state, hv->reset, sizeof(int) * 2, hipMemcpyHostToDevice, st));
  DecodeOpts rows; rows.rows_streams = B;
  for (int p0 = p_start; p0 <= p_end; p0 += L) {
    const int l = std::min(L, p_end - p0 + 1);
    const size_t off = (size_t)(p0 - p_start) * B;
    c->dec_key_bound = key_bound(p0 + l, c->P);
    rows.ids = c->row_ids + off;
    int r = decode_core(c, l * B, st, rows);
    if (r != TW_OK) return r;
    SamplerArgs sa = sa0;
    sa.B = l * B; sa.rows_streams = B; sa.row_pos0 = p0; sa.row_lastts = c->row_lastts + off; sa.row_choice = c->row_choice + off;
    sa.row_last_pos = p_end; sa.row_is_last = (p0 + l > p_end) ? 1 : 0; sa.verify_state = c->verify_state;
    if (ba) {
      SeqBiasArgs b = *ba;
      b.rows = l * B; b.rows_streams = B; b.row_pos0 = p0;
      HIPCHK(c, launch_seq_bias(b, st));
    }
    if (ra) {
      RepeatArgs rp = *ra;
      rp.rows = l * B; rp.rows_streams = B; rp.row_pos0 = p0;
      HIPCHK(c, launch_repeat(rp, st));
    }
    HIPCHK(c, launch_sampler_rows(sa, st));
    HIPCHK(c, hipMemcpyAsync(hv, c->verify_state, sizeof(int) * (2 + B), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ++c->last_draft[2];
    if (hv->decided != 0) {
      const int pn = hv->decided;
      if (pn < p0 + 1 || pn > p0 + l) return fail(c, TW_EHIP, "verify: decided position %d outside the launch [%d, %d)", pn - 1, p0, p0 + l);
      bool same = pn <= p_given;
      for (int b = 0; b < B; ++b) {
        same = same && tok[(size_t)b * ld + pn] == hv->choice[b];
        tok[(size_t)b * ld + pn] = hv->choice[b];
      }
      *next_given = same ? 1 : 0;
      *p_next = pn;
      return TW_OK;
    }
  }
  return fail(c, TW_EHIP, "verify: the round ended without a decision");
}

// words of the packed sequence-bias table at its capacities: header | grp_off | grp_tok | seq_off | bias | tokens
constexpr size_t kSeqBiasTabWords = kSeqBiasHeader + 2 * (size_t)TW_BIAS_MAX_SEQS + 2 * ((size_t)TW_BIAS_MAX_SEQS + 1) + TW_BIAS_MAX_TOKENS;

// Checks a tw_bias_opts (every TW_EINVAL of tw_generate_greedy_biased) and packs it into the table seq_bias_kernel reads (tw_common.h:
// SeqBiasArgs): per stream the sequences grouped by last token, a group's length-1 member first, then the caller's order; groups in
// the order their last token first appears.  Host work only.
int pack_seq_bias(tw_ctx* c, int B, const tw_bias_opts* bo, std::vector<int>& tab) {
  const char* fn = "tw_generate_greedy_biased";
  const int S = bo->n_seq;
  if (S < 0 || S > TW_BIAS_MAX_SEQS) return fail(c, TW_EINVAL, "%s: %d sequences (at most %d)", fn, S, TW_BIAS_MAX_SEQS);
  if (!bo->row_off || !bo->seq_off || !bo->tokens || !bo->bias) return fail(c, TW_EINVAL, "%s: null array in tw_bias_opts", fn);
  if (bo->row_off[0] != 0 || bo->row_off[B] != S) return fail(c, TW_EINVAL, "%s: row_off must run from 0 to n_seq", fn);
  for (int b = 0; b < B; ++b)
    if (bo->row_off[b + 1] < bo->row_off[b]) return fail(c, TW_EINVAL, "%s: row_off decreases at row %d", fn, b);
  if (bo->seq_off[0] != 0) return fail(c, TW_EINVAL, "%s: seq_off must start at 0", fn);
  for (int i = 0; i < S; ++i) {
    const long long L = (long long)bo->seq_off[i + 1] - bo->seq_off[i];
    if (L < 1 || L > TW_BIAS_MAX_SEQ_LEN) return fail(c, TW_EINVAL, "%s: sequence %d has %lld tokens (1 .. %d)", fn, i, L, TW_BIAS_MAX_SEQ_LEN);
    if (bo->seq_off[i + 1] > TW_BIAS_MAX_TOKENS) return fail(c, TW_EINVAL, "%s: more than %d tokens", fn, TW_BIAS_MAX_TOKENS);
    if (!std::isfinite(bo->bias[i])) return fail(c, TW_EINVAL, "%s: the bias of sequence %d is NaN or infinite", fn, i);
  }
  const int n_tok = bo->seq_off[S];
  for (int i = 0; i < n_tok; ++i)
    if (bo->tokens[i] < 0 || bo->tokens[i] >= c->V) return fail(c, TW_EINVAL, "%s: token %d outside the vocabulary", fn, bo->tokens[i]);
  std::vector<int> strm(65, 0), grp_off(1, 0), grp_tok, seq_off(1, 0), tokens;
  std::vector<float> bias;
  for (int b = 0; b < B; ++b) {
    std::set<std::vector<int>> seen;
    std::map<int, size_t> group_of;                 // last token -> index into members
    std::vector<std::vector<int>> members;          // per group: sequence indices in summation order
    std::vector<int> last_of;
    for (int i = bo->row_off[b]; i < bo->row_off[b + 1]; ++i) {
      const int* t = bo->tokens + bo->seq_off[i];
      const int L = bo->seq_off[i + 1] - bo->seq_off[i];
      if (!seen.insert(std::vector<int>(t, t + L)).second) return fail(c, TW_EINVAL, "%s: row %d lists sequence %d twice", fn, b, i);
      auto it = group_of.find(t[L - 1]);
      if (it == group_of.end()) {
        it = group_of.emplace(t[L - 1], members.size()).first;
        members.emplace_back();
        last_of.push_back(t[L - 1]);
      }
      std::vector<int>& m = members[it->second];
      if (L == 1) m.insert(m.begin(), i); else m.push_back(i);
    }
    strm[b] = (int)grp_tok.size();
    for (size_t g = 0; g < members.size(); ++g) {
      grp_tok.push_back(last_of[g]);
      for (int i : members[g]) {
        tokens.insert(tokens.end(), bo->tokens + bo->seq_off[i], bo->tokens + bo->seq_off[i + 1]);
        seq_off.push_back((int)tokens.size());
        bias.push_back(bo->bias[i]);
      }
      grp_off.push_back((int)bias.size());
    }
  }
  for (int b = B; b < 65; ++b) strm[b] = (int)grp_tok.size();
  tab.assign(kSeqBiasHeader, 0);
  for (int b = 0; b < 65; ++b) tab[kSeqBiasStreamOff + b] = strm[b];
  auto append = [&](int slot, const int* p, size_t n) { tab[slot] = (int)tab.size(); tab.insert(tab.end(), p, p + n); };
  append(0, grp_off.data(), grp_off.size());
  append(1, grp_tok.data(), grp_tok.size());
  append(2, seq_off.data(), seq_off.size());
  append(3, reinterpret_cast<const int*>(bias.data()), bias.size());
  append(4, tokens.data(), tokens.size());
  if (tab.size() > kSeqBiasTabWords) return fail(c, TW_EINVAL, "%s: the packed table exceeds its capacity", fn);   // (cannot happen)
  return TW_OK;
}

// Checks a tw_repeat_opts for `rows` rows (every TW_EINVAL of tw_generate_greedy_repeat; max_n: the largest n-gram size) and fills the
// table repeat_kernel reads (tw_common.h: RepeatArgs).  *any = some row has an option on.  Host work only.
int pack_repeat(tw_ctx* c, const char* fn, int rows, int max_n, const tw_repeat_opts* ro, int* tab, bool* any) {
  if (rows < 1 || rows > 64) return fail(c, TW_EINVAL, "%s: %d rows (1..64)", fn, rows);
  if (ro->penalty_ignore < 0) return fail(c, TW_EINVAL, "%s: penalty_ignore %d < 0", fn, ro->penalty_ignore);
  *any = false;
  for (int b = 0; b < 64; ++b) {
    const float r = (b < rows && ro->penalty) ? ro->penalty[b] : 1.0f;
    const int N = (b < rows && ro->no_repeat_ngram) ? ro->no_repeat_ngram[b] : 0;
    if (!std::isfinite(r) || !(r > 0.f)) return fail(c, TW_EINVAL, "%s: the penalty of row %d is NaN, infinite or <= 0", fn, b);
    if (N < 0 || N > max_n) return fail(c, TW_EINVAL, "%s: no_repeat_ngram[%d] = %d outside [0, %d]", fn, b, N, max_n);
    memcpy(tab + b, &r, sizeof r);
    tab[64 + b] = N;
    *any |= r != 1.0f || N != 0;
  }
  tab[128] = ro->penalty_ignore;
  for (int i = 129; i < kRepeatTabWords; ++i) tab[i] = 0;
  return TW_OK;
}

int reset_state(tw_ctx* c, int n_prompt, hipStream_t st) {
  c->h_pinned->state = DecState{0, n_prompt, 0, 0};
  HIPCHK(c, hipMemcpyAsync(c->stt, &c->h_pinned->state, sizeof(DecState), hipMemcpyHostToDevice, st));
  return TW_OK;
}

// Every TW_EINVAL of the logits processors' options, for every tw_generate_* call and tw_score_tokens alike (include/thewhisper.h)
int check_processor_opts(tw_ctx* c, const tw_greedy_opts* o) {
  if (o->n_begin_suppress < 0 || o->n_begin_suppress > 64 || o->n_suppress < 0 || o->n_suppress > 1024 ||
      (o->n_begin_suppress > 0 && !o->begin_suppress) || (o->n_suppress > 0 && !o->suppress))
    return fail(c, TW_EINVAL, "suppress lists too long");
  if (o->pad_id < 0 || o->pad_id >= c->V || o->eos_id < 0 || o->eos_id >= c->V)
    return fail(c, TW_EINVAL, "pad_id %d / eos_id %d outside the vocabulary", o->pad_id, o->eos_id);   // (the sampler embeds pad_id for finished rows)
  return TW_OK;
}

// The two suppress lists of `o` (checked; nullptr: none) through h_stage to their device arrays, and the static list as a bitmap
int upload_suppress_lists(tw_ctx* c, const tw_greedy_opts* o, int* bsup_dev, int* sup_dev, unsigned* bits, hipStream_t st) {
  const int n_bsup = o ? o->n_begin_suppress : 0, n_sup = o ? o->n_suppress : 0;
  if (n_bsup > 0) {
    memcpy(c->h_stage->bsup, o->begin_suppress, sizeof(int) * n_bsup);
    HIPCHK(c, hipMemcpyAsync(bsup_dev, c->h_stage->bsup, sizeof(int) * n_bsup, hipMemcpyHostToDevice, st));
  }
  if (n_sup > 0) {
    memcpy(c->h_stage->sup, o->suppress, sizeof(int) * n_sup);
    HIPCHK(c, hipMemcpyAsync(sup_dev, c->h_stage->sup, sizeof(int) * n_sup, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, launch_suppress_bitmap(sup_dev, n_sup, bits, c->V, st));
  return TW_OK;
}

// A device table of `cap` ints and its pinned staging, both allocated by the first call of the context that needs them and freed in
// tw_destroy: the first n ints of src go up (the staging is not touched again before the call's stream synchronisation)
int upload_first_use_table(tw_ctx* c, int*& dev, int*& pinned, size_t cap, bool zero, const int* src, size_t n, hipStream_t st) {
  if (!dev) ALLOC(c, dev, sizeof(int) * cap, zero);
  if (!pinned) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&pinned), sizeof(int) * cap));
  memcpy(pinned, src, sizeof(int) * n);
  HIPCHK(c, hipMemcpyAsync(dev, pinned, sizeof(int) * n, hipMemcpyHostToDevice, st));
  return TW_OK;
}

}  // namespace

extern "C" {

int tw_decoder_reset(tw_ctx* c, int32_t B, void* stream) {
  if (!c) return TW_EINVAL;
  TW_ON_DEVICE(c);
  if (B < 1 || B > c->cross_B) return fail(c, TW_ESTATE, "tw_decoder_reset: B=%d but cross K/V holds %d clips", B, c->cross_B);
  hipStream_t st = pick_stream(c, stream);
  int r = reset_state(c, 0, st);
  if (r != TW_OK) return r;
  c->dec_key_bound = c->P;
  HIPCHK(c, hipStreamSynchronize(st));
  return TW_OK;
}

int tw_decode_step(tw_ctx* c, int32_t B, const int32_t* ids_host, float* logits_dev, void* stream) {
  if (!c || !ids_host) return fail(c, TW_EINVAL, "tw_decode_step: null argument");
  TW_ON_DEVICE(c);
  if (B < 1 || B > c->cross_B) return fail(c, TW_ESTATE, "tw_decode_step: B=%d but cross K/V holds %d clips", B, c->cross_B);
  hipStream_t st = pick_stream(c, stream);
  HIPCHK(c, hipMemcpyAsync(c->cur_ids, ids_host, sizeof(int) * B, hipMemcpyHostToDevice, st));
  int r = decode_core(c, B, st);
  if (r != TW_OK) return r;
  if (logits_dev)
    HIPCHK(c, hipMemcpyAsync(logits_dev, c->logits, sizeof(float) * (size_t)B * c->V, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, launch_advance(c->stt, 1, st));  // pos += 1 on the device (keeps the step graph-compatible)
  return TW_OK;
}

// The generation loop of tw_generate_greedy and tw_generate_sample.  so == nullptr: the greedy call, launch for launch what it has always
// issued.  so != nullptr (validated by tw_generate_sample: no forced / draft tokens, finite temperatures, a live row): every step's
// sampler is launch_sample; rows with temperature < 0 start finished.  fo != nullptr (validated by tw_generate_sample_filtered, which
// hands it on only when some sampled row has a filter on): every step's sampler is launch_sample_filtered.  bo != nullptr
// (tw_generate_greedy_biased, greedy only, n_seq > 0): launch_seq_bias runs in front of every sampler launch, rows mode included.
// ro != nullptr (tw_generate_greedy_repeat, greedy only; dropped here when every row is off): launch_repeat runs behind it.
// n_pad != nullptr (tw_generate_greedy_ragged, which validated it: plain greedy only, no forced / draft tokens, some row padded): every
// step is a ragged step (decode_core) that embeds its own input, so the sampler writes no next input row.
static int generate_loop(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const tw_sample_opts* so,
                         const tw_filter_opts* fo, const tw_bias_opts* bo, int32_t* out_ids, int32_t* out_len, void* stream,
                         const int32_t* n_pad = nullptr, const tw_repeat_opts* ro = nullptr) {
  const bool ragged = n_pad != nullptr, biased = bo != nullptr;
  // the call's flavour: its name in messages, and its character in the step-graph key - the sampler's launches, or 'r', a ragged call,
  // whose steps are other launches: a graph of one flavour is never replayed for a call of another
  const char* fn = ragged ? "tw_generate_greedy_ragged" : ro ? "tw_generate_greedy_repeat" : biased ? "tw_generate_greedy_biased" : fo ? "tw_generate_sample_filtered" : so ? "tw_generate_sample" : "tw_generate_greedy";
  char flavour = ragged ? 'r'                         : ro ? (biased ? 'q' : 'p')         : biased ? 'b'                         : fo ? 'f'                           : so ? 's'                  : 'g';
  if (ragged && (so || fo || bo || ro || o->n_forced != 0 || o->n_draft != 0)) return fail(c, TW_EINVAL, "%s: padding goes with the plain greedy call only", fn);
  if (B < 1 || B > c->cross_B) return fail(c, TW_ESTATE, "%s: B=%d but cross K/V holds %d clips", fn, B, c->cross_B);
  if (n_prompt < 1 || n_prompt >= c->P) return fail(c, TW_EINVAL, "bad n_prompt %d", n_prompt);
  int r = check_processor_opts(c, o);
  if (r != TW_OK) return r;
  if (o->want_alignment && c->Ha == 0) return fail(c, TW_EINVAL, "want_alignment but the context has no alignment heads");
  // forced output tokens (tw_greedy_opts::n_forced): the begin index of the generation is n_begin, the tokens behind it are given
  const int n_forced = o->n_forced;
  if (n_forced < 0 || n_forced >= n_prompt) return fail(c, TW_EINVAL, "bad n_forced %d (n_prompt %d)", n_forced, n_prompt);
  // draft tokens (tw_greedy_opts::n_draft): guesses of the output, verified - the result is the plain call's, token for token
  const int n_draft = o->n_draft;
  if (n_draft < 0 || n_draft >= n_prompt || (n_draft > 0 && n_forced > 0))
    return fail(c, TW_EINVAL, "bad n_draft %d (n_prompt %d, n_forced %d: one of the two)", n_draft, n_prompt, n_forced);
  const int n_begin = n_prompt - n_forced - n_draft;
  int max_len = n_begin + o->max_new_tokens;
  if (o->max_length > 0 && o->max_length < max_len) max_len = o->max_length;
  if (max_len > c->P) max_len = c->P;
  if (max_len <= n_prompt) return fail(c, TW_EINVAL, "nothing to generate (max_len %d <= n_prompt %d)", max_len, n_prompt);
  const int out_ld = o->max_length > 0 ? o->max_length : max_len;
  std::vector<int> bias_tab;   // the call's packed sequence table (checked here, with the other refusals; uploaded with the initial state)
  if (biased) {
    if (B > 64) return fail(c, TW_EINVAL, "%s: %d streams (1..64)", fn, B);
    r = pack_seq_bias(c, B, bo, bias_tab);
    if (r != TW_OK) return r;
  }
  int repeat_tab[kRepeatTabWords];   // the call's per-stream penalties and n-gram sizes (checked here; uploaded with the initial state)
  bool repeat = false;
  if (ro) {
    if (so || fo) return fail(c, TW_EINVAL, "%s: repeat options go with the greedy call only", fn);
    r = pack_repeat(c, fn, B, c->P, ro, repeat_tab, &repeat);
    if (r != TW_OK) return r;
    if (!repeat) flavour = biased ? 'b' : 'g';   // every row off: the call is the plain or the biased one
  }
  c->dec_key_bound = max_len;   // per step: the 64-key bucket of the position (below)
  hipStream_t st = pick_stream(c, stream);
  const int P = c->P;

  // ---- initial state: staged in PINNED memory, so the uploads are asynchronous and the loop's first launch follows them without a
  //      host synchronisation (the staging area is not touched again before the stream synchronisation at the end of this call) ----
  GenStage& hs = *c->h_stage;
  int* hseq = c->h_seq;                                    // [B][P]
  for (size_t i = 0; i < (size_t)B * P; ++i) hseq[i] = o->pad_id;
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < n_prompt; ++i) {
      const int t = prompt[(size_t)b * n_prompt + i];
      if (t < 0 || t >= c->V) return fail(c, TW_EINVAL, "prompt token %d out of range", t);
      hseq[(size_t)b * P + i] = t;
    }
    // with forced tokens the loop starts at the LAST given position (everything before it is prefilled below)
    hs.first[b] = prompt[(size_t)b * n_prompt + (n_forced > 0 ? n_prompt - 1 : 0)];
    hs.finished0[b] = (so && so->temperature[b] < 0.f) ? 1 : 0;   // a row that sits the call out starts finished
    hs.last_ts0[b] = -1;
    if (so) {
      const float t = so->temperature[b];
      hs.noisy[b] = t > 0.f ? 1 : 0;
      hs.inv_t[b] = t > 0.f ? 1.0f / t : 1.0f;
      const uint64_t sd = so->seed ? so->seed[b] : 0, of = so->offset ? so->offset[b] : 0;
      hs.key[b][0] = (uint32_t)sd; hs.key[b][1] = (uint32_t)(sd >> 32);
      hs.off[b][0] = (uint32_t)of; hs.off[b][1] = (uint32_t)(of >> 32);
      if (fo) {   // (a greedy row ignores the filters: its arg-max is always kept)
        hs.top_k[b] = (t > 0.f && fo->top_k) ? fo->top_k[b] : 0;
        hs.top_p[b] = (t > 0.f && fo->top_p) ? fo->top_p[b] : 1.0f;
      }
    }
    for (int i = n_begin; i < n_prompt; ++i) {   // state the sampler would have after producing the forced tokens itself
      const int t = prompt[(size_t)b * n_prompt + i];
      if (t == o->eos_id) return fail(c, TW_EINVAL, n_draft > 0 ? "a draft token is <eos>" : "a forced token is <eos>");
      if (n_forced > 0 && o->timestamps && t > o->no_timestamps_id) hs.last_ts0[b] = t;
    }
  }
  // the call's tables, each allocated by the context's first call of that flavour (upload_first_use_table)
  if (biased) r = upload_first_use_table(c, c->bias_tab, c->h_bias, kSeqBiasTabWords, false, bias_tab.data(), bias_tab.size(), st);
  if (r == TW_OK && repeat) r = upload_first_use_table(c, c->repeat_tab, c->h_repeat, kRepeatTabWords, true, repeat_tab, kRepeatTabWords, st);
  if (r == TW_OK && ragged) {
    int pads[64] = {};
    std::copy(n_pad, n_pad + B, pads);
    r = upload_first_use_table(c, c->n_pad_tab, c->h_n_pad, 64, true, pads, 64, st);
  }
  if (r != TW_OK) return r;
  HIPCHK(c, hipMemcpyAsync(c->seq, hseq, sizeof(int) * (size_t)B * P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->cur_ids, hs.first, sizeof(int) * B, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->finished, hs.finished0, sizeof(int) * B, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->last_ts, hs.last_ts0, sizeof(int) * B, hipMemcpyHostToDevice, st));
  if (so) {
    HIPCHK(c, hipMemcpyAsync(c->sample_inv_t, hs.inv_t, sizeof(float) * B, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->sample_key, hs.key, sizeof(uint32_t) * 2 * B, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->sample_off, hs.off, sizeof(uint32_t) * 2 * B, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->sample_noisy, hs.noisy, sizeof(int) * B, hipMemcpyHostToDevice, st));
  }
  if (fo) {
    HIPCHK(c, hipMemcpyAsync(c->filter_top_k, hs.top_k, sizeof(int) * B, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->filter_top_p, hs.top_p, sizeof(float) * B, hipMemcpyHostToDevice, st));
  }
  r = upload_suppress_lists(c, o, c->begin_suppress_dev, c->suppress_dev, c->suppress_bits, st);
  if (r != TW_OK) return r;
  hs.state = DecState{0, n_begin, max_len - 1, B};
  HIPCHK(c, hipMemcpyAsync(c->stt, &hs.state, sizeof(DecState), hipMemcpyHostToDevice, st));
  int s_start = n_forced > 0 ? n_prompt - 1 : 0;
  if (n_forced > 0) {   // positions 0 .. n_prompt-2 in batched launches (self-attention caches + alignment rows); device pos -> s_start
    r = prefill_core(c, B, prompt, n_prompt, s_start, st);
    if (r != TW_OK) return r;
  }

  SamplerArgs sa{};
  sa.logits = c->logits; sa.V = c->V; sa.B = B; sa.seq = c->seq; sa.seq_ld = P; sa.cur_ids = c->cur_ids;
  sa.finished = c->finished; sa.last_ts = c->last_ts; sa.stt = c->stt;
  sa.eos = o->eos_id; sa.pad = o->pad_id; sa.min_new = o->min_new_tokens; sa.timestamps = o->timestamps;
  sa.no_ts_id = o->no_timestamps_id; sa.max_initial_ts = o->max_initial_timestamp_index;
  sa.begin_suppress = c->begin_suppress_dev; sa.n_begin_suppress = o->n_begin_suppress;
  sa.suppress_bits = c->suppress_bits; sa.partials = c->sampler_partials;
  SeqBiasArgs ba{};   // the table lives in context-owned device memory: one captured graph serves every list
  ba.logits = c->logits; ba.V = c->V; ba.rows = B; ba.seq = c->seq; ba.seq_ld = P; ba.finished = c->finished; ba.stt = c->stt; ba.tab = c->bias_tab;
  RepeatArgs rpa{};   // ... and every penalty and n-gram size
  rpa.logits = c->logits; rpa.V = c->V; rpa.rows = B; rpa.seq = c->seq; rpa.seq_ld = P; rpa.finished = c->finished; rpa.stt = c->stt; rpa.tab = c->repeat_tab;
  // the embedding of the token a step has chosen is written by the sampler's last launch (k_decode.hip: embed_row), so a step is
  // layers + logits + sampler; only the FIRST step of the call needs its input row from a launch of its own
  c->last_draft[0] = n_draft * B; c->last_draft[1] = c->last_draft[2] = c->last_draft[3] = 0;
  c->last_prompt_rows[0] = c->last_prompt_rows[1] = 0;
  if (n_forced > 0) {   // the batched prefill above (prefill_core)
    const int per_launch = std::max(1, rows_per_launch(c) / B);
    c->last_prompt_rows[0] = (s_start + per_launch - 1) / per_launch; c->last_prompt_rows[1] = s_start;
  }
  // The plain greedy call takes its prompt as ONE rows-mode launch (below, behind the timer's start) when the prompt's rows fit one:
  // every other flavour - and a longer prompt or more streams - consumes it one position per step
  const bool prompt_rows = !so && !fo && !biased && !repeat && !ragged && n_forced == 0 && n_draft == 0 && n_prompt >= 2 &&
                           n_prompt * B <= rows_per_launch(c) && (size_t)n_prompt * B <= c->row_ids_cap;
  bool draft_all_done = false;
  if (n_draft > 0) {
    // ---- draft-and-verify: rounds of rows-mode launches over the given tokens (verify_round), then the ordinary loop from where the
    //      last round stopped.  Round 1 takes everything that was offered (prompt included: its positions have to be processed anyway);
    //      after a rejection the REST of the draft is offered again at the same positions (a changed timestamp or word usually leaves
    //      the text behind it as it was), in launches of one group of rows - such a launch costs about what one step costs and
    //      yields at least the one token a step yields - until a round confirms nothing or the draft is used up.
    //      The rounds also end as soon as ANY stream's token at `pos` is <eos>: rows mode has no finished rows (sampler_mask samples
    //      every row, sampler_rows_finish_kernel rewrites every finished flag), so another round would feed that <eos> as an input
    //      and decode the stream on.  At this exit the device state is the loop's - finished[] is set for exactly the streams
    //      that hold <eos> at `pos`, since no earlier round ended on one - and the ordinary loop pads those rows from here;
    //      the other streams' remaining guesses are dropped. ----
    constexpr int first_rows = 64, retry_rows = 16, max_rounds = 16;   // rows of round 1 / of a retry launch, rounds per call
    const int cap = rows_per_launch(c);
    if (B > cap) return fail(c, TW_EINVAL, "n_draft: %d streams exceed the %d rows of a launch", B, cap);
    const int ts_begin = o->timestamps ? o->no_timestamps_id + 1 : c->V;
    const int p_end = n_prompt - 1;
    tic(c, 3, st);
    int pos = 0, rounds = 0;
    while (true) {
      // (several streams: at least four positions per retry launch, or a round could not confirm anything)
      const int rows = rounds == 0 ? std::min(cap, std::max(first_rows, B)) : std::min(cap, std::max(retry_rows, 4 * B));
      const int pe = rounds == 0 ? p_end : std::min(p_end, pos + std::max(1, rows / B) - 1);
      int pn = 0, next_given = 0;
      r = verify_round(c, B, hseq, P, n_begin, ts_begin, pos, pe, rows, sa, st, &pn, p_end, &next_given, biased ? &ba : nullptr, repeat ? &rpa : nullptr);
      if (r != TW_OK) return r;
      ++rounds;
      // guesses this round confirmed: the given tokens at positions <= p_acc that were compared, and the token the round produced
      // itself at p_acc + 1 where it is the guess that stood there (a round that ends without a mismatch before the draft does)
      const int confirmed = pn - 1 - std::max(pos, n_begin - 1) + ((next_given && pn >= n_begin) ? 1 : 0);
      c->last_draft[1] += std::max(0, confirmed) * B;
      pos = pn;
      draft_all_done = true;
      bool any_done = false;
      for (int b = 0; b < B; ++b) {
        const bool done = pos >= n_begin && hseq[(size_t)b * P + pos] == o->eos_id;
        draft_all_done &= done;
        any_done |= done;
      }
      if (any_done || pos > p_end - 1 || pos >= max_len - 1 || rounds >= max_rounds || (rounds > 1 && confirmed <= 0)) break;
    }
    c->last_draft[3] = rounds;
    s_start = pos;
  }
  sa.tok_emb = c->tok_emb; sa.pos_emb = c->dec_pos; sa.x_next = ragged ? nullptr : c->dx0; sa.d = c->d; sa.dtype = c->dtype;
  DecodeOpts step; step.embed = false; step.n_pad = ragged ? c->n_pad_tab : nullptr;   // the loop's step: its input rows are in place, or - ragged - it embeds its own
  // (a prompt taken as rows: the sampler behind the rows launch writes the loop's first input row, below)
  if (!ragged && !prompt_rows) HIPCHK(c, launch_embed(c->dtype, c->cur_ids, c->stt, c->tok_emb, c->dec_pos, c->dx0, B, c->d, 0, st));

  // ---- graph replay: one captured step per self-attention length bucket, captured on first use ----
  char keybuf[256];
  // (last field: the call's flavour, above - greedy, biased greedy, greedy with repeat options 'p', biased with repeat options 'q',
  //  sampling, filtered sampling, ragged greedy)
  snprintf(keybuf, sizeof keybuf, "%d|%d|%d|%d|%d|%d|%d|%d|%d|%c", B, o->eos_id, o->pad_id, o->min_new_tokens, o->timestamps,
           o->no_timestamps_id, o->max_initial_timestamp_index, o->n_begin_suppress, o->n_suppress, flavour);
  SampleArgs sma{};   // the per-row arrays live in device memory: one captured graph serves every temperature and seed
  sma.inv_t = c->sample_inv_t; sma.key = c->sample_key; sma.off = c->sample_off; sma.noisy = c->sample_noisy; sma.parts = c->sample_parts;
  FilterArgs fla{};   // ... and every top-k / top-p
  fla.top_k = c->filter_top_k; fla.top_p = c->filter_top_p; fla.choice = c->filter_choice;
  auto sample_step = [&]() -> hipError_t {
    if (biased) {
      hipError_t e = launch_seq_bias(ba, st);
      if (e != hipSuccess) return e;
    }
    if (repeat) {
      hipError_t e = launch_repeat(rpa, st);
      if (e != hipSuccess) return e;
    }
    if (!so) return launch_sampler(sa, st);
    sma.s = sa;
    if (!fo) return launch_sample(sma, st);
    fla.sm = sma;
    return launch_sample_filtered(fla, st);
  };
  const bool use_graph = c->cfg.use_graph != 0;
  if (use_graph && c->step_graph_key != keybuf) {   // other options: the captured sampler arguments are stale
    for (auto& kv : c->step_graphs) (void)hipGraphExecDestroy(kv.second);
    c->step_graphs.clear();
    c->step_graph_key = keybuf;
  }
  // `n` consecutive steps per graph (the step is position-independent: the position lives in device memory): fewer graph
  // launches for the host to issue when a step is short (turbo, one stream: 0.2 ms)
  auto graph_for = [&](int kb, int n, hipGraphExec_t* out) -> int {
    const std::string k = std::to_string(kb) + "x" + std::to_string(n);
    auto it = c->step_graphs.find(k);
    if (it != c->step_graphs.end()) { *out = it->second; return TW_OK; }
    hipGraph_t g = nullptr;
    c->dec_key_bound = kb;
    HIPCHK(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int r = TW_OK;
    hipError_t es = hipSuccess;
    for (int i = 0; i < n && r == TW_OK && es == hipSuccess; ++i) {
      r = decode_core(c, B, st, step);
      if (r == TW_OK) es = sample_step();
    }
    hipError_t ee = hipStreamEndCapture(st, &g);
    if (r != TW_OK) { if (g) (void)hipGraphDestroy(g); return r; }
    if (es != hipSuccess || ee != hipSuccess) {
      if (g) (void)hipGraphDestroy(g);
      return fail(c, TW_EHIP, "decode-step graph capture failed: %s", hipGetErrorString(es != hipSuccess ? es : ee));
    }
    hipGraphExec_t ex = nullptr;
    hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) return fail(c, TW_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
    c->step_graphs[k] = ex;
    *out = ex;
    return TW_OK;
  };

  // ---- the loop: step s consumes position s and produces the token at position s+1 ----
  static const bool host_timing = getenv("TW_HOST_TIMING") != nullptr;   // where the CALL's wall time goes besides the device loop
  const auto ht0 = std::chrono::steady_clock::now();
  auto ht_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ht0).count(); };
  double ht_first = 0, ht_loop = 0;
  if (n_draft == 0) tic(c, 3, st);
  if (prompt_rows) {
    // ---- the prompt as rows: positions 0 .. n_prompt - 1 of every stream in one rows-mode launch - the shape of a verify_round with
    //      nothing to verify - instead of n_prompt steps: the weights are streamed once, the cross attention reads a stream's K / V^T
    //      once (k_decode.hip: dec_cross_attn_rows_kernel), and the sampler runs for the LAST position only, as the ordinary
    //      sampler on that position's rows of the logits.  A row's bits do not depend on the rows that share its launch, and the
    //      sampler of a prompt position changes nothing but the device position, so the token at n_prompt, the self caches, the
    //      alignment rows, finished[], last_ts[] and the position are the step path's; the loop goes on from position n_prompt. ----
    fill_row_tables(c, B, hseq, P, 0, n_prompt - 1, false, 0, 0);
    HIPCHK(c, hipMemcpyAsync(c->row_ids, c->h_rows.tok, sizeof(int) * (size_t)n_prompt * B, hipMemcpyHostToDevice, st));
    DecodeOpts rows; rows.rows_streams = B; rows.ids = c->row_ids;
    c->dec_key_bound = key_bound(n_prompt, max_len);
    r = decode_core(c, n_prompt * B, st, rows);
    if (r != TW_OK) return r;
    HIPCHK(c, launch_advance(c->stt, n_prompt - 1, st));
    SamplerArgs sl = sa;
    sl.logits = c->logits + (size_t)(n_prompt - 1) * B * c->V;
    HIPCHK(c, launch_sampler(sl, st));
    c->last_prompt_rows[0] = 1; c->last_prompt_rows[1] = n_prompt;
    s_start = n_prompt;
  }
  // two steps per graph launch: measured +2 % at one turbo stream, +0.3 % at 16 large-v3 streams (4 per launch: +3 % / +0.8 %, but
  // up to 7 steps past the last <eos> instead of 5); the finished flags are read LAG launches behind so the host never waits
  constexpr int group = 2;
  // while <eos> is still masked (min_new_tokens not reached) no stream can finish, so nothing is wasted by replaying more steps per
  // launch: 8 at a time there (forced-length decoding, e.g. RTFx runs with a fixed token budget); the reference backend's calls
  // set no minimum and always take the small group
  constexpr int group_forced = 8;
  const int LAG = std::max(1, 4 / group);
  int steps = 0, launches = 0;
  bool all_done = draft_all_done;
  for (int s = s_start; s < max_len - 1 && !all_done;) {
    // step s produces the token at position s + 1, which can be <eos> only once s + 1 - n_prompt >= min_new_tokens
    // (not for the first launch of a call: submitting a graph costs host time in proportion to its nodes, and the GPU is idle until
    // the first one is in; a small first launch covers the submission of the big second one)
    const bool eos_free = use_graph && launches >= 1 && group_forced > group && s + group_forced <= max_len - 1 &&
                          s + group_forced - 1 < n_begin + o->min_new_tokens - 1;
    const int n = eos_free ? group_forced : ((use_graph && s + group <= max_len - 1) ? group : 1);   // steps in this launch
    const int last = s + n - 1;
    const int kb = key_bound(last + 1, max_len);   // keys [0, kb) cover positions s .. last
    if (use_graph) {
      hipGraphExec_t ex = nullptr;
      int r = graph_for(kb, n, &ex);
      if (r != TW_OK) return r;
      HIPCHK(c, hipGraphLaunch(ex, st));
    } else {
      c->dec_key_bound = kb;
      int r = decode_core(c, B, st, step);
      if (r != TW_OK) return r;
      HIPCHK(c, sample_step());
    }
    steps += n;
    s += n;
    const int slot = launches % 8;
    HIPCHK(c, hipMemcpyAsync(c->h_pinned->finished[slot], c->finished, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipEventRecord(c->ring_ev[slot], st));
    if (launches >= LAG) {
      const int ps = (launches - LAG) % 8;
      HIPCHK(c, hipEventSynchronize(c->ring_ev[ps]));
      bool done = true;
      for (int b = 0; b < B; ++b) done &= (c->h_pinned->finished[ps][b] != 0);
      all_done = done;
    }
    if (launches == 0) ht_first = ht_ms();
    ++launches;
  }
  toc(c, 3, st);
  ht_loop = ht_ms();
  c->last_steps = steps + (prompt_rows ? n_prompt : 0);   // positions consumed by the call, the prompt's as steps or as rows
  HIPCHK(c, hipMemcpyAsync(hseq, c->seq, sizeof(int) * (size_t)B * P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (host_timing) {
    float dev_ms = 0.f;
    (void)hipEventElapsedTime(&dev_ms, c->ev0[3], c->ev1[3]);
    fprintf(stderr, "TW_HOST_TIMING generate B=%d steps=%d launches=%d: first launch submitted at %.3f ms, host loop done at %.3f ms, "
                    "synchronised at %.3f ms; device loop (events) %.3f ms\n", B, steps, launches, ht_first, ht_loop, ht_ms(), dev_ms);
  }

  // common sequence length exactly as HF's loop would have stopped: when the last row hit eos, or at max_len
  const int produced = s_start + steps + 1;  // positions 0 .. s_start + steps are filled
  // first position a SAMPLED token sits at (forced / confirmed draft tokens before it are never <eos>; unconfirmed draft tokens
  // behind `produced` are stale and never looked at).  The draft rounds end at the first <eos> of ANY stream, so a stream's <eos>
  // sits at s_start or behind it, never in front
  const int scan_from = n_draft > 0 ? std::max(s_start, n_begin) : n_prompt;
  int L = scan_from + 1;
  for (int b = 0; b < B; ++b) {
    if (so && so->temperature[b] < 0.f) continue;   // a row that sat the call out holds pad_id only: it does not set the length
    int lb = produced;
    for (int i = scan_from; i < produced; ++i)
      if (hseq[(size_t)b * P + i] == o->eos_id) { lb = i + 1; break; }
    if (lb > L) L = lb;
  }
  for (int b = 0; b < B; ++b) {
    bool ended = false;
    for (int i = 0; i < out_ld; ++i) {
      int v = o->pad_id;
      if (i < L) {
        v = hseq[(size_t)b * P + i];
        if (ended) v = o->pad_id;
        if (i >= scan_from && v == o->eos_id) ended = true;
      }
      out_ids[(size_t)b * out_ld + i] = v;
    }
  }
  *out_len = L;
  c->last_seq_len = L;
  c->last_n_prompt = n_prompt;
  return TW_OK;
}

int tw_generate_greedy(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o,
                       int32_t* out_ids, int32_t* out_len, void* stream) {
  if (!c || !prompt || !o || !out_ids || !out_len) return fail(c, TW_EINVAL, "tw_generate_greedy: null argument");
  TW_ON_DEVICE(c);
  return generate_loop(c, B, prompt, n_prompt, o, nullptr, nullptr, nullptr, out_ids, out_len, stream);
}

int tw_generate_greedy_biased(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const tw_bias_opts* bo,
                              int32_t* out_ids, int32_t* out_len, void* stream) {
  if (!c || !prompt || !o || !out_ids || !out_len) return fail(c, TW_EINVAL, "tw_generate_greedy_biased: null argument");
  TW_ON_DEVICE(c);
  // nothing to add: the call IS tw_generate_greedy, launch for launch
  return generate_loop(c, B, prompt, n_prompt, o, nullptr, nullptr, (bo && bo->n_seq != 0) ? bo : nullptr, out_ids, out_len, stream);
}

int tw_generate_greedy_repeat(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const tw_bias_opts* bo,
                              const tw_repeat_opts* ro, int32_t* out_ids, int32_t* out_len, void* stream) {
  if (!c || !prompt || !o || !out_ids || !out_len) return fail(c, TW_EINVAL, "tw_generate_greedy_repeat: null argument");
  TW_ON_DEVICE(c);
  if (ro && B > 64) return fail(c, TW_EINVAL, "tw_generate_greedy_repeat: %d streams (1..64)", B);
  // ro == nullptr, or every row off (generate_loop finds out while it checks the values): the call IS tw_generate_greedy(_biased)
  return generate_loop(c, B, prompt, n_prompt, o, nullptr, nullptr, (bo && bo->n_seq != 0) ? bo : nullptr, out_ids, out_len, stream, nullptr, ro);
}

int tw_generate_greedy_ragged(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const int32_t* n_pad,
                              int32_t* out_ids, int32_t* out_len, void* stream) {
  const char* fn = "tw_generate_greedy_ragged";
  if (!c || !prompt || !o || !out_ids || !out_len) return fail(c, TW_EINVAL, "%s: null argument", fn);
  TW_ON_DEVICE(c);
  bool padded = false;
  if (B > 64) return fail(c, TW_EINVAL, "%s: %d streams (1..64)", fn, B);
  if (n_pad) {
    for (int b = 0; b < B; ++b) {
      if (n_pad[b] < 0 || n_pad[b] >= n_prompt)   // (a row needs one real token)
        return fail(c, TW_EINVAL, "%s: n_pad[%d] = %d outside [0, n_prompt = %d)", fn, b, n_pad[b], n_prompt);
      padded |= n_pad[b] > 0;
    }
  }
  if (padded && (o->n_forced != 0 || o->n_draft != 0))
    return fail(c, TW_EINVAL, "%s: n_forced %d / n_draft %d: forced and draft tokens do not go with padded rows", fn, o->n_forced, o->n_draft);
  // nothing padded: the call IS tw_generate_greedy, launch for launch
  return generate_loop(c, B, prompt, n_prompt, o, nullptr, nullptr, nullptr, out_ids, out_len, stream, padded ? n_pad : nullptr);
}

// Word offsets of the beam state tables inside tw_ctx::beam_tab / h_beam (tw_common.h: BeamArgs); rows are beam-major, k * n_clips + c
namespace {
constexpr size_t kBeamRunScore = 0, kBeamFinScore = 64, kBeamFinFlag = 128, kBeamFinLen = 192, kBeamOpen = 256, kBeamDone = 320,
                 kBeamIdx = 384, kBeamPen = 448 /* 576 words */, kBeamFinSeq = 1024;
size_t beam_tab_words(const tw_ctx* c) { return kBeamFinSeq + (size_t)64 * c->P; }
}  // namespace

// The beam loop (THE RULE: include/thewhisper.h).  Not captured: a beam step is issued launch by launch in use_graph contexts too, so
// the two settings run the same launches, and the captured greedy step graphs of the context are left alone.
// tw_generate_beam (aligned_entry false: want_alignment is refused) and tw_generate_beam_aligned; fn names the caller in messages
static int generate_beam_checked(const char* fn, bool aligned_entry, tw_ctx* c, int32_t n, const int32_t* prompt, int32_t n_prompt,
                                 const tw_greedy_opts* o, const tw_beam_opts* bo, int32_t* out_ids, int32_t* out_len, float* out_score,
                                 int32_t* out_nbest_ids, float* out_nbest_score, int32_t* out_hyp_len, void* stream) {
  if (!c || !prompt || !o || !bo || !out_ids || !out_len) return fail(c, TW_EINVAL, "%s: null argument", fn);
  TW_ON_DEVICE(c);
  const int K = bo->num_beams;
  if (K < 2 || K > kBeamMax) return fail(c, TW_EINVAL, "%s: num_beams %d outside 2..%d", fn, K, kBeamMax);
  if (n < 1 || (long long)n * K > c->Bmax || n * K > 64)
    return fail(c, TW_EINVAL, "%s: %d clips x %d beams exceed max_batch %d (or 64 rows)", fn, n, K, c->Bmax);
  if (!std::isfinite(bo->length_penalty)) return fail(c, TW_EINVAL, "%s: length_penalty is NaN or infinite", fn);
  if (bo->early_stopping != 0 && bo->early_stopping != 1) return fail(c, TW_EINVAL, "%s: early_stopping %d outside {0, 1}", fn, bo->early_stopping);
  if ((o->want_alignment && !aligned_entry) || o->n_forced != 0 || o->n_draft != 0)
    return fail(c, TW_EINVAL, "%s: want_alignment, n_forced and n_draft do not go with beams", fn);
  if (o->want_alignment != 0 && o->want_alignment != 1) return fail(c, TW_EINVAL, "%s: want_alignment %d outside {0, 1}", fn, o->want_alignment);
  const bool rec = o->want_alignment != 0;   // record the alignment rows and the ancestry; gather behind the loop
  if (rec && c->Ha == 0) return fail(c, TW_EINVAL, "%s: want_alignment but the context has no alignment heads", fn);
  if (c->w8) return fail(c, TW_EINVAL, "%s: fp8 contexts are not supported", fn);
  if (c->P > kBeamSeqMax) return fail(c, TW_EINVAL, "%s: target_positions %d above %d", fn, c->P, kBeamSeqMax);
  if (n > c->cross_B) return fail(c, TW_ESTATE, "%s: %d clips but cross K/V holds %d", fn, n, c->cross_B);
  if (n_prompt < 1 || n_prompt >= c->P) return fail(c, TW_EINVAL, "bad n_prompt %d", n_prompt);
  int r = check_processor_opts(c, o);
  if (r != TW_OK) return r;
  int max_len = n_prompt + o->max_new_tokens;
  if (o->max_length > 0 && o->max_length < max_len) max_len = o->max_length;
  if (max_len > c->P) max_len = c->P;
  if (max_len <= n_prompt) return fail(c, TW_EINVAL, "nothing to generate (max_len %d <= n_prompt %d)", max_len, n_prompt);
  const int out_ld = o->max_length > 0 ? o->max_length : max_len;
  for (size_t i = 0; i < (size_t)n * n_prompt; ++i)
    if (prompt[i] < 0 || prompt[i] >= c->V) return fail(c, TW_EINVAL, "prompt token %d out of range", prompt[i]);
  hipStream_t st = pick_stream(c, stream);
  const int P = c->P, rows = n * K;
  const size_t words = beam_tab_words(c);
  if (!c->beam_tab) ALLOC(c, c->beam_tab, sizeof(int) * words, true);
  if (!c->beam_parts) ALLOC(c, c->beam_parts, sizeof(BeamPartial) * 64 * 32, true);
  if (!c->h_beam) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_beam), sizeof(int) * words));
  if (rec && !c->beam_anc) ALLOC(c, c->beam_anc, sizeof(int) * ((size_t)kBeamSeqMax * 64 + 64), true);

  // ---- initial state, staged in pinned memory (not touched again before the synchronisation at the end of the call) ----
  GenStage& hs = *c->h_stage;
  int* hseq = c->h_seq;   // [rows][P]
  int* hb = c->h_beam;
  float* hbf = reinterpret_cast<float*>(hb);
  memset(hb, 0, sizeof(int) * kBeamFinSeq);
  for (int k = 0; k < K; ++k)
    for (int b = 0; b < n; ++b) {
      const int row = k * n + b;
      for (int i = 0; i < P; ++i) hseq[(size_t)row * P + i] = hb[kBeamFinSeq + (size_t)row * P + i] = i < n_prompt ? prompt[(size_t)b * n_prompt + i] : o->pad_id;
      hs.first[row] = prompt[(size_t)b * n_prompt];
      hs.finished0[row] = 0;
      hs.last_ts0[row] = -1;
      hbf[kBeamRunScore + row] = k == 0 ? 0.f : -1e9f;
      hbf[kBeamFinScore + row] = -1e9f;
      hb[kBeamFinLen + row] = n_prompt;
      hb[kBeamIdx + row] = k;
      hb[kBeamOpen + b] = 1;
    }
  for (int g = 0; g <= P; ++g) hbf[kBeamPen + g] = (float)std::pow((double)g, (double)bo->length_penalty);
  HIPCHK(c, hipMemcpyAsync(c->beam_tab, hb, sizeof(int) * (kBeamFinSeq + (size_t)rows * P), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->seq, hseq, sizeof(int) * (size_t)rows * P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->cur_ids, hs.first, sizeof(int) * rows, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->finished, hs.finished0, sizeof(int) * rows, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->last_ts, hs.last_ts0, sizeof(int) * rows, hipMemcpyHostToDevice, st));
  r = upload_suppress_lists(c, o, c->begin_suppress_dev, c->suppress_dev, c->suppress_bits, st);
  if (r != TW_OK) return r;
  hs.state = DecState{0, n_prompt, max_len - 1, rows};
  HIPCHK(c, hipMemcpyAsync(c->stt, &hs.state, sizeof(DecState), hipMemcpyHostToDevice, st));
  // every clip's cross K / V for its beams 1 .. K-1: slots n .. n K - 1 (the clips' own slots are only read)
  const size_t ckv_e = c->esz;
  HIPCHK(c, launch_beam_cross_copy(c->cross_k, c->cross_v, (long long)((size_t)c->Bmax * c->Tp * c->d * ckv_e),
                                   (long long)((size_t)c->Tp * c->d * ckv_e), c->Ld, n, K, st));
  c->cross_B = n;   // the slots behind the clips now hold their copies

  BeamArgs ba{};
  SamplerArgs& sa = ba.s;
  sa.logits = c->logits; sa.V = c->V; sa.B = rows; sa.seq = c->seq; sa.seq_ld = P; sa.cur_ids = c->cur_ids;
  sa.finished = c->finished; sa.last_ts = c->last_ts; sa.stt = c->stt;
  sa.eos = o->eos_id; sa.pad = o->pad_id; sa.min_new = o->min_new_tokens; sa.timestamps = o->timestamps;
  sa.no_ts_id = o->no_timestamps_id; sa.max_initial_ts = o->max_initial_timestamp_index;
  sa.begin_suppress = c->begin_suppress_dev; sa.n_begin_suppress = o->n_begin_suppress;
  sa.suppress_bits = c->suppress_bits; sa.partials = c->sampler_partials;
  ba.n_clips = n; ba.K = K; ba.early = bo->early_stopping; ba.max_len = max_len; ba.parts = c->beam_parts;
  float* tf = reinterpret_cast<float*>(c->beam_tab);
  ba.run_score = tf + kBeamRunScore; ba.fin_score = tf + kBeamFinScore; ba.pen = tf + kBeamPen;
  ba.fin_flag = c->beam_tab + kBeamFinFlag; ba.fin_len = c->beam_tab + kBeamFinLen; ba.open = c->beam_tab + kBeamOpen;
  ba.done = c->beam_tab + kBeamDone; ba.beam_idx = c->beam_tab + kBeamIdx; ba.fin_seq = c->beam_tab + kBeamFinSeq;
  if (rec) {
    ba.back = c->beam_anc; ba.fin_last = c->beam_anc + (size_t)kBeamSeqMax * 64;
    HIPCHK(c, hipMemsetAsync(ba.fin_last, 0, sizeof(int) * 64, st));
  }

  const int Pp = (P + 63) / 64 * 64;
  // embeds from cur_ids; without want_alignment the alignment rows of an earlier call stay as they are, with it every beam's rows
  // are recorded where the beam sits (prompt steps included) and gathered along the ancestry once the loop is over
  DecodeOpts step; step.record_alignment = rec;
  tic(c, 3, st);
  constexpr int LAG = 2;
  int steps = 0;
  bool all_done = false;
  for (int s = 0; s < max_len - 1 && !all_done; ++s) {
    const bool in_prompt = s + 1 < n_prompt;   // the step only appends the next prompt token: no logits, nothing to reorder
    const int kb = key_bound(s + 1, max_len);
    c->dec_key_bound = kb;
    step.logits = !in_prompt;
    r = decode_core(c, rows, st, step);
    if (r != TW_OK) return r;
    HIPCHK(c, launch_beam_step(ba, in_prompt, st));
    if (!in_prompt)
      HIPCHK(c, launch_beam_reorder(c->dtype, c->self_k, c->self_v, (long long)c->Bmax * Pp * c->d, (long long)Pp * c->d, (long long)Pp * 64,
                                    c->Ld, c->H, kb, ba, st));
    HIPCHK(c, launch_advance(c->stt, 1, st));
    ++steps;
    const int slot = s % 8;
    HIPCHK(c, hipMemcpyAsync(c->h_pinned->finished[slot], ba.done, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipEventRecord(c->ring_ev[slot], st));
    if (s >= LAG) {
      const int ps = (s - LAG) % 8;
      HIPCHK(c, hipEventSynchronize(c->ring_ev[ps]));
      bool done = true;
      for (int b = 0; b < n; ++b) done &= (c->h_pinned->finished[ps][b] != 0);
      all_done = done;
    }
  }
  toc(c, 3, st);
  c->last_steps = steps;
  if (rec) HIPCHK(c, launch_beam_align_gather(c->align, c->Ha, P, c->T, max_len - 1, ba, st));
  HIPCHK(c, hipMemcpyAsync(hb, c->beam_tab, sizeof(int) * (kBeamFinSeq + (size_t)rows * P), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));

  // ---- results: hypothesis i of clip b is finished row i * n + b; everything behind its end is pad_id ----
  int L_best = n_prompt, L_all = n_prompt;
  for (int b = 0; b < n; ++b)
    for (int k = 0; k < K; ++k) {
      const int len = std::min(std::max(hb[kBeamFinLen + k * n + b], n_prompt), max_len);
      if (k == 0) L_best = std::max(L_best, len);
      L_all = std::max(L_all, len);
    }
  auto emit = [&](int row, int32_t* dst) {
    const int len = std::min(std::max(hb[kBeamFinLen + row], n_prompt), max_len);
    for (int i = 0; i < out_ld; ++i) dst[i] = i < len ? hb[kBeamFinSeq + (size_t)row * P + i] : o->pad_id;
  };
  for (int b = 0; b < n; ++b) {
    emit(b, out_ids + (size_t)b * out_ld);
    if (out_score) out_score[b] = hbf[kBeamFinScore + b];
    for (int k = 0; k < K; ++k) {
      if (out_nbest_ids) emit(k * n + b, out_nbest_ids + ((size_t)b * K + k) * out_ld);
      if (out_nbest_score) out_nbest_score[(size_t)b * K + k] = hbf[kBeamFinScore + k * n + b];
      if (out_hyp_len) out_hyp_len[(size_t)b * K + k] = std::min(std::max(hb[kBeamFinLen + k * n + b], n_prompt), max_len);
    }
  }
  out_len[0] = L_best;   // (two entries, always: the header says so)
  out_len[1] = L_all;
  c->last_seq_len = L_best;
  c->last_n_prompt = n_prompt;
  return TW_OK;
}

int tw_generate_beam(tw_ctx* c, int32_t n, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const tw_beam_opts* bo,
                     int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_nbest_ids, float* out_nbest_score, void* stream) {
  return generate_beam_checked("tw_generate_beam", false, c, n, prompt, n_prompt, o, bo, out_ids, out_len, out_score, out_nbest_ids,
                               out_nbest_score, nullptr, stream);
}

int tw_generate_beam_aligned(tw_ctx* c, int32_t n, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const tw_beam_opts* bo,
                             int32_t* out_ids, int32_t* out_len, float* out_score, int32_t* out_nbest_ids, float* out_nbest_score,
                             int32_t* out_hyp_len, void* stream) {
  return generate_beam_checked("tw_generate_beam_aligned", true, c, n, prompt, n_prompt, o, bo, out_ids, out_len, out_score, out_nbest_ids,
                               out_nbest_score, out_hyp_len, stream);
}

// tw_generate_sample and tw_generate_sample_filtered (fn names the caller in messages); fo == nullptr: no filter
static int generate_sample_checked(const char* fn, tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o,
                                   const tw_sample_opts* so, const tw_filter_opts* fo, int32_t* out_ids, int32_t* out_len, void* stream) {
  if (!c || !prompt || !o || !so || !so->temperature || !so->seed || !out_ids || !out_len)
    return fail(c, TW_EINVAL, "%s: null argument", fn);
  TW_ON_DEVICE(c);
  if (B < 1 || B > 64) return fail(c, TW_EINVAL, "%s: %d streams (1..64)", fn, B);
  if (o->n_forced != 0 || o->n_draft != 0)
    return fail(c, TW_EINVAL, "%s: n_forced %d / n_draft %d: forced and draft tokens are for greedy calls", fn, o->n_forced, o->n_draft);
  bool live = false;
  for (int b = 0; b < B; ++b) {
    const float t = so->temperature[b];
    if (!std::isfinite(t) || (t > 0.f && !std::isfinite(1.0f / t)))   // (a subnormal T: 1 / T overflows and the noise would be lost)
      return fail(c, TW_EINVAL, "%s: temperature of row %d is not finite, or too small for 1 / T to be", fn, b);
    live |= t >= 0.f;
  }
  if (!live) return fail(c, TW_EINVAL, "%s: every row has a negative temperature (nothing to generate)", fn);
  bool filtered = false;   // a filter is on in a row that samples
  if (fo) {
    for (int b = 0; b < B; ++b) {
      const int k = fo->top_k ? fo->top_k[b] : 0;
      const float p = fo->top_p ? fo->top_p[b] : 1.0f;
      if (k < 0) return fail(c, TW_EINVAL, "%s: negative top_k %d of row %d (0 = off)", fn, k, b);
      if (!(p > 0.f && p <= 1.0f)) return fail(c, TW_EINVAL, "%s: top_p %g of row %d is NaN or outside (0, 1] (1 = off)", fn, (double)p, b);
      filtered |= so->temperature[b] > 0.f && (k > 0 || p < 1.0f);
    }
  }
  if (filtered && c->V > kFilterMaxVocab)
    return fail(c, TW_EINVAL, "%s: the filter kernel holds %d ids, the vocabulary has %d", fn, kFilterMaxVocab, c->V);
  return generate_loop(c, B, prompt, n_prompt, o, so, filtered ? fo : nullptr, nullptr, out_ids, out_len, stream);
}

int tw_generate_sample(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o, const tw_sample_opts* so,
                       int32_t* out_ids, int32_t* out_len, void* stream) {
  return generate_sample_checked("tw_generate_sample", c, B, prompt, n_prompt, o, so, nullptr, out_ids, out_len, stream);
}

int tw_generate_sample_filtered(tw_ctx* c, int32_t B, const int32_t* prompt, int32_t n_prompt, const tw_greedy_opts* o,
                                const tw_sample_opts* so, const tw_filter_opts* fo, int32_t* out_ids, int32_t* out_len, void* stream) {
  return generate_sample_checked("tw_generate_sample_filtered", c, B, prompt, n_prompt, o, so, fo, out_ids, out_len, stream);
}

int tw_score_tokens(tw_ctx* c, int32_t B, const int32_t* ids, int32_t ld, int32_t seq_len, int32_t n_prompt, const tw_greedy_opts* o,
                    int32_t no_speech_id, int32_t no_speech_pos, float* out_logprob, float* out_logprob_raw, float* out_no_speech,
                    void* stream) {
  if (!c || !ids) return fail(c, TW_EINVAL, "tw_score_tokens: null argument");
  TW_ON_DEVICE(c);
  const int P = c->P;
  const int cap = rows_per_launch(c);
  if (B < 1 || B > cap) return fail(c, TW_EINVAL, "tw_score_tokens: %d streams, a launch has %d rows", B, cap);
  if (n_prompt < 1 || seq_len <= n_prompt || seq_len > P) return fail(c, TW_EINVAL, "tw_score_tokens: seq_len %d outside (n_prompt %d, %d]", seq_len, n_prompt, P);
  if (ld < seq_len) return fail(c, TW_EINVAL, "tw_score_tokens: ld %d < seq_len %d", ld, seq_len);
  const int n_pos = seq_len - 1;    // position p yields the score of the token at p + 1
  if ((size_t)n_pos * B > c->row_ids_cap) return fail(c, TW_EINVAL, "tw_score_tokens: %d positions x %d streams exceed the row table", n_pos, B);
  if (!o && out_logprob) return fail(c, TW_EINVAL, "tw_score_tokens: the masked log-probabilities need the processors' options");
  int r = o ? check_processor_opts(c, o) : TW_OK;
  if (r != TW_OK) return r;
  if (no_speech_id >= c->V) return fail(c, TW_EINVAL, "tw_score_tokens: no_speech_id %d outside the vocabulary", no_speech_id);
  if (no_speech_id >= 0 && (no_speech_pos < 0 || no_speech_pos >= seq_len - 1))
    return fail(c, TW_EINVAL, "tw_score_tokens: no_speech_pos %d outside [0, %d)", no_speech_pos, seq_len - 1);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < seq_len; ++i) {
      const int t = ids[(size_t)b * ld + i];
      if (t < 0 || t >= c->V) return fail(c, TW_EINVAL, "tw_score_tokens: token %d out of range", t);
    }
  if (B > c->cross_B) return fail(c, TW_ESTATE, "tw_score_tokens: B=%d but cross K/V holds %d clips", B, c->cross_B);
  hipStream_t st = pick_stream(c, stream);

  // ---- staging (pinned; not touched again before the synchronisation at the end of this call) ----
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < P; ++i) c->h_seq[(size_t)b * P + i] = i < seq_len ? ids[(size_t)b * ld + i] : 0;
  // the rows' tokens, and per row the last timestamp token among the tokens sampled so far
  fill_row_tables(c, B, ids, ld, 0, n_pos - 1, true, n_prompt, (o && o->timestamps) ? o->no_timestamps_id + 1 : c->V);
  HIPCHK(c, hipMemcpyAsync(c->score_seq, c->h_seq, sizeof(int) * (size_t)B * P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->row_ids, c->h_rows.tok, sizeof(int) * (size_t)n_pos * B, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->row_lastts, c->h_rows.lastts, sizeof(int) * (size_t)n_pos * B, hipMemcpyHostToDevice, st));
  r = upload_suppress_lists(c, o, c->score_bsup, c->score_sup, c->score_bits, st);
  if (r == TW_OK) r = reset_state(c, n_prompt, st);     // device position 0, begin index n_prompt
  if (r != TW_OK) return r;

  ScoreArgs a{};
  a.s.logits = c->logits; a.s.V = c->V; a.s.seq = c->score_seq; a.s.seq_ld = P; a.s.stt = c->stt;
  a.s.begin_suppress = c->score_bsup; a.s.n_begin_suppress = o ? o->n_begin_suppress : 0; a.s.suppress_bits = c->score_bits;
  a.s.max_initial_ts = -1;
  if (o) {   // (NULL: nothing is masked and the masked numbers, equal to the raw ones, are not handed out)
    a.s.eos = o->eos_id; a.s.pad = o->pad_id; a.s.min_new = o->min_new_tokens; a.s.timestamps = o->timestamps;
    a.s.no_ts_id = o->no_timestamps_id; a.s.max_initial_ts = o->max_initial_timestamp_index;
  }
  a.parts = c->score_parts; a.out_masked = c->score_out.masked; a.out_raw = c->score_out.raw; a.out_ld = P;
  a.ns_id = no_speech_id >= 0 ? no_speech_id : -1; a.ns_pos = no_speech_pos; a.out_ns = c->score_out.no_speech;

  // ---- positions 0 .. seq_len-2 in rows-mode launches with logits (B streams x L consecutive positions), each scored at once ----
  const int key_bound_before = c->dec_key_bound;
  const int L = std::max(1, cap / B);
  DecodeOpts rows; rows.rows_streams = B; rows.record_alignment = false;
  for (int p0 = 0; p0 < n_pos; p0 += L) {
    const int l = std::min(L, n_pos - p0);
    const size_t off = (size_t)p0 * B;
    c->dec_key_bound = key_bound(p0 + l, P);
    rows.ids = c->row_ids + off;
    r = decode_core(c, l * B, st, rows);
    if (r != TW_OK) { c->dec_key_bound = key_bound_before; return r; }
    a.s.B = l * B; a.s.rows_streams = B; a.s.row_pos0 = p0; a.s.row_lastts = c->row_lastts + off;
    HIPCHK(c, launch_score_rows(a, st));
    HIPCHK(c, launch_advance(c->stt, l, st));
  }
  c->dec_key_bound = key_bound_before;
  HIPCHK(c, hipMemcpyAsync(c->h_score.masked, c->score_out.masked, sizeof(float) * c->score_floats, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));

  // ---- [B, seq_len]: 0 for the prompt and for the padding behind a row's first <eos> (the <eos> itself is scored) ----
  for (int b = 0; b < B; ++b) {
    int last = seq_len - 1;
    if (o)
      for (int i = n_prompt; i < seq_len; ++i)
        if (ids[(size_t)b * ld + i] == o->eos_id) { last = i; break; }
    for (int i = 0; i < seq_len; ++i) {
      const bool scored = i >= n_prompt && i <= last;
      if (out_logprob) out_logprob[(size_t)b * seq_len + i] = scored ? c->h_score.masked[(size_t)b * P + i] : 0.f;
      if (out_logprob_raw) out_logprob_raw[(size_t)b * seq_len + i] = scored ? c->h_score.raw[(size_t)b * P + i] : 0.f;
    }
    if (no_speech_id >= 0 && out_no_speech) out_no_speech[b] = c->h_score.no_speech[b];
  }
  return TW_OK;
}

int tw_last_draft(tw_ctx* c, int32_t* offered, int32_t* accepted, int32_t* launches, int32_t* rounds) {
  if (!c) return TW_EINVAL;
  if (offered) *offered = c->last_draft[0];
  if (accepted) *accepted = c->last_draft[1];
  if (launches) *launches = c->last_draft[2];
  if (rounds) *rounds = c->last_draft[3];
  return TW_OK;
}

int tw_last_prompt_rows(tw_ctx* c, int32_t* launches, int32_t* positions) {
  if (!c) return TW_EINVAL;
  if (launches) *launches = c->last_prompt_rows[0];
  if (positions) *positions = c->last_prompt_rows[1];
  return TW_OK;
}

int tw_get_alignment(tw_ctx* c, int32_t B, int32_t n_rows, float* out_host, void* stream) {
  if (!c || !out_host) return TW_EINVAL;
  TW_ON_DEVICE(c);
  if (c->Ha == 0) return fail(c, TW_EINVAL, "context has no alignment heads");
  if (B < 1 || B > c->Bmax || n_rows < 1 || n_rows > c->P) return fail(c, TW_EINVAL, "bad B/n_rows");
  hipStream_t st = pick_stream(c, stream);
  const size_t T = c->T, P = c->P, Ha = c->Ha;
  for (int b = 0; b < B; ++b)
    for (size_t h = 0; h < Ha; ++h)
      HIPCHK(c, hipMemcpyAsync(out_host + ((size_t)b * Ha + h) * n_rows * T, c->align + ((size_t)b * Ha + h) * P * T,
                               sizeof(float) * n_rows * T, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return TW_OK;
}

int tw_set_alignment(tw_ctx* c, int32_t B, int32_t n_rows, const float* in_host, void* stream) {
  if (!c || !in_host) return TW_EINVAL;
  TW_ON_DEVICE(c);
  if (c->Ha == 0) return fail(c, TW_EINVAL, "context has no alignment heads");
  if (B < 1 || B > c->Bmax || n_rows < 1 || n_rows > c->P) return fail(c, TW_EINVAL, "bad B/n_rows");
  hipStream_t st = pick_stream(c, stream);
  const size_t T = c->T, P = c->P, Ha = c->Ha;
  for (int b = 0; b < B; ++b)
    for (size_t h = 0; h < Ha; ++h)
      HIPCHK(c, hipMemcpyAsync(c->align + ((size_t)b * Ha + h) * P * T, in_host + ((size_t)b * Ha + h) * n_rows * T,
                               sizeof(float) * n_rows * T, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return TW_OK;
}

// Columns of the alignment matrix a stream keeps (num_frames NULL: all T).  HF crops with the Python slice
// `weights[..., : num_frames // 2]` (HF:models/whisper/generation_whisper.py:346-349): floor division, and a NEGATIVE bound
// (num_frames - seek < 0 happens in the seek loop for clips shorter than the chunk) counts from the end.  Reproduced literally so
// token timestamps stay identical to the reference.
static int kept_columns(int T, const int32_t* num_frames) {
  int nc = T;
  if (num_frames) {
    const int nf = *num_frames;
    nc = (nf >= 0) ? nf / 2 : -((-nf + 1) / 2);   // floor(nf / 2)
    if (nc < 0) nc += T;
  }
  if (nc > T) nc = T;
  if (nc < 0) nc = 0;    // nothing left: HF's DTW on the empty matrix puts every token at time index -1 (dtw_kernel)
  return nc;
}

int tw_token_timestamps(tw_ctx* c, int32_t B, int32_t n_prompt, int32_t seq_len, const int32_t* num_frames_host,
                        double time_precision, float* out_ts_host, void* stream) {
  if (!c || !out_ts_host) return fail(c, TW_EINVAL, "tw_token_timestamps: null argument");
  TW_ON_DEVICE(c);
  if (c->Ha == 0) return fail(c, TW_EINVAL, "context has no alignment heads");
  if (B < 1 || B > c->Bmax || seq_len < 2 || seq_len > c->P || n_prompt < 1 || n_prompt >= seq_len)
    return fail(c, TW_EINVAL, "bad B/n_prompt/seq_len (%d,%d,%d)", B, n_prompt, seq_len);
  hipStream_t st = pick_stream(c, stream);
  std::vector<int> cols(B);
  for (int b = 0; b < B; ++b) cols[b] = kept_columns(c->T, num_frames_host ? &num_frames_host[b] : nullptr);
  HIPCHK(c, hipMemcpy(c->n_cols, cols.data(), sizeof(int) * B, hipMemcpyHostToDevice));
  DtwArgs a{};
  a.align = c->align; a.Ha = c->Ha; a.P = c->P; a.T = c->T; a.B = B; a.n_prompt = n_prompt; a.n_rows = seq_len - 1;
  a.n_cols = c->n_cols; a.median_width = 7; a.zbuf = c->zbuf; a.mat = c->mat; a.trace = c->trace; a.out_ts = c->out_ts;
  // the reference multiplies int64 frame indices by the Python float 0.02 (float64)
  a.time_precision = time_precision;
  tic(c, 4, st);
  HIPCHK(c, launch_token_timestamps(a, st));
  toc(c, 4, st);
  HIPCHK(c, hipMemcpyAsync(out_ts_host, c->out_ts, sizeof(float) * (size_t)B * seq_len, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return TW_OK;
}

int tw_token_timestamps_each(tw_ctx* c, int32_t B, int32_t n_prompt, const int32_t* seq_len_host, int32_t ld, const int32_t* num_frames_host,
                             double time_precision, float* out_ts_host, void* stream) {
  const char* fn = "tw_token_timestamps_each";
  if (!c || !out_ts_host || !seq_len_host) return fail(c, TW_EINVAL, "%s: null argument", fn);
  TW_ON_DEVICE(c);
  if (c->Ha == 0) return fail(c, TW_EINVAL, "context has no alignment heads");
  if (B < 1 || B > c->Bmax || ld < 1 || n_prompt < 1) return fail(c, TW_EINVAL, "%s: bad B/n_prompt/ld (%d,%d,%d)", fn, B, n_prompt, ld);
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    if (seq_len_host[b] < 0 || seq_len_host[b] > ld || seq_len_host[b] > c->P)
      return fail(c, TW_EINVAL, "%s: seq_len[%d] = %d outside [0, min(ld = %d, target_positions = %d)]", fn, b, seq_len_host[b], ld, c->P);
    longest = std::max(longest, seq_len_host[b]);
  }
  hipStream_t st = pick_stream(c, stream);
  if (!c->dtw_len) ALLOC(c, c->dtw_len, sizeof(int) * c->Bmax, true);
  std::vector<int> cols(B);
  for (int b = 0; b < B; ++b) cols[b] = kept_columns(c->T, num_frames_host ? &num_frames_host[b] : nullptr);
  HIPCHK(c, hipMemcpy(c->n_cols, cols.data(), sizeof(int) * B, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->dtw_len, seq_len_host, sizeof(int) * B, hipMemcpyHostToDevice));
  const int dld = std::min((int)ld, c->P + 1);   // entries per row on the device (out_ts holds P + 1); the rest repeats on the host
  DtwArgs a{};
  a.align = c->align; a.Ha = c->Ha; a.P = c->P; a.T = c->T; a.B = B; a.n_prompt = n_prompt; a.n_rows = std::max(longest, n_prompt + 1) - 1;
  a.n_cols = c->n_cols; a.median_width = 7; a.zbuf = c->zbuf; a.mat = c->mat; a.trace = c->trace; a.out_ts = c->out_ts;
  a.time_precision = time_precision;
  a.row_len = c->dtw_len; a.out_ld = dld;
  if (a.n_rows + 1 > c->P) a.n_rows = c->P - 1;   // (n_prompt >= target_positions: every row then has N_b <= 0)
  tic(c, 4, st);
  HIPCHK(c, launch_token_timestamps(a, st));
  toc(c, 4, st);
  if (dld == ld) {
    HIPCHK(c, hipMemcpyAsync(out_ts_host, c->out_ts, sizeof(float) * (size_t)B * ld, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  } else {
    std::vector<float> tmp((size_t)B * dld);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), c->out_ts, sizeof(float) * tmp.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < ld; ++k) out_ts_host[(size_t)b * ld + k] = tmp[(size_t)b * dld + std::min(k, dld - 1)];
  }
  return TW_OK;
}

int tw_last_timings(tw_ctx* c, float* ms_out5, int32_t* steps_out) {
  if (!c || !ms_out5) return TW_EINVAL;
  TW_ON_DEVICE(c);
  for (int i = 0; i < 5; ++i) {
    ms_out5[i] = -1.f;
    if (c->ev_valid[i]) {
      float ms = 0.f;
      if (hipEventSynchronize(c->ev1[i]) == hipSuccess && hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]) == hipSuccess)
        ms_out5[i] = ms;
    }
  }
  if (steps_out) *steps_out = c->last_steps;
  return TW_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// HIP streams / events owned by THIS library's runtime (the one torch mapped): used by the host-side stage overlap
// (thewhisper_amd/overlap.py) so that no second copy of libamdhip64 is ever dlopen'ed by name.
// ---------------------------------------------------------------------------------------------
extern "C" {

int tw_vad_energy(int32_t device, const float* pcm_dev, int64_t stream_stride, int32_t B, int32_t n_frames, float* state_dev,
                  float* prob_dev, void* stream) {
  if (!pcm_dev || !state_dev || !prob_dev || B < 1 || n_frames < 1 || stream_stride < (int64_t)n_frames * 512) return TW_EINVAL;
  if ((reinterpret_cast<uintptr_t>(pcm_dev) & 15) || (stream_stride & 3)) return TW_EINVAL;   // 16-byte frame loads
  DeviceGuard guard(device);
  hipError_t e = launch_vad_energy(pcm_dev, stream_stride, B, n_frames, state_dev, prob_dev, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) { g_create_error = std::string("vad_energy_kernel: ") + hipGetErrorString(e); return TW_EHIP; }
  return TW_OK;
}

int tw_repeat_logits(int32_t device, float* logits_dev, int32_t V, int32_t rows, const int32_t* hist_host, int32_t ld,
                     const int32_t* n_hist_host, const tw_repeat_opts* ro, void* stream) {
  const char* fn = "tw_repeat_logits";
  if (!logits_dev || !hist_host || !n_hist_host || !ro) return fail(nullptr, TW_EINVAL, "%s: null argument", fn);
  if (V < 1 || ld < 0 || ld > kRepeatMaxHist) return fail(nullptr, TW_EINVAL, "%s: V = %d, ld = %d (ld at most %d)", fn, V, ld, kRepeatMaxHist);
  // staging: history [rows][ld] | n_hist [rows] | table
  std::vector<int> h;
  bool any = false;
  {
    int tab[kRepeatTabWords];
    int r = pack_repeat(nullptr, fn, rows, kRepeatMaxHist, ro, tab, &any);
    if (r != TW_OK) return r;
    h.resize((size_t)rows * ld + rows + kRepeatTabWords);
    for (int i = 0; i < rows; ++i) {
      const int n = n_hist_host[i];
      if (n < 0 || n > ld) return fail(nullptr, TW_EINVAL, "%s: n_hist[%d] = %d outside [0, %d]", fn, i, n, ld);
      for (int j = 0; j < ld; ++j) {
        const int t = hist_host[(size_t)i * ld + j];
        if (j < n && (t < 0 || t >= V)) return fail(nullptr, TW_EINVAL, "%s: history id %d of row %d outside [0, %d)", fn, t, i, V);
        h[(size_t)i * ld + j] = j < n ? t : 0;
      }
      h[(size_t)rows * ld + i] = n;
    }
    memcpy(h.data() + (size_t)rows * ld + rows, tab, sizeof tab);
  }
  DeviceGuard guard(device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int* dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), sizeof(int) * h.size());
  if (e != hipSuccess) return fail(nullptr, TW_ENOMEM, "%s: hipMalloc failed: %s", fn, hipGetErrorString(e));
  e = hipMemcpyAsync(dev, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_repeat_logits(logits_dev, V, rows, dev, ld, dev + (size_t)rows * ld, dev + (size_t)rows * ld + rows, st);
  const hipError_t es = hipStreamSynchronize(st);
  (void)hipFree(dev);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(nullptr, TW_EHIP, "%s: %s", fn, hipGetErrorString(e));
  return TW_OK;
}

}  // extern "C"

namespace {
// the refusals tw_language_logits and tw_detect_language share (include/thewhisper.h)
int check_lang_list(tw_ctx* c, const char* fn, const int32_t* ids, int32_t n_lang, int32_t V) {
  if (!ids) return fail(c, TW_EINVAL, "%s: null argument", fn);
  if (n_lang < 1 || n_lang > TW_LANG_MAX) return fail(c, TW_EINVAL, "%s: n_lang = %d outside 1 .. %d", fn, n_lang, TW_LANG_MAX);
  int sorted[TW_LANG_MAX];
  for (int j = 0; j < n_lang; ++j) {
    if (ids[j] < 0 || ids[j] >= V) return fail(c, TW_EINVAL, "%s: language id %d outside [0, %d)", fn, ids[j], V);
    sorted[j] = ids[j];
  }
  std::sort(sorted, sorted + n_lang);
  for (int j = 1; j < n_lang; ++j)
    if (sorted[j] == sorted[j - 1]) return fail(c, TW_EINVAL, "%s: language id %d is listed twice", fn, sorted[j]);
  return TW_OK;
}
}  // namespace

extern "C" {

int tw_language_logits(int32_t device, const float* logits_dev, int32_t V, int32_t rows, const int32_t* lang_ids_host, int32_t n_lang,
                       int32_t* out_id_host, float* out_prob_host, void* stream) {
  const char* fn = "tw_language_logits";
  if (!logits_dev || !lang_ids_host || !out_id_host) return fail(nullptr, TW_EINVAL, "%s: null argument", fn);
  if (V < 1 || rows < 1 || rows > 65535) return fail(nullptr, TW_EINVAL, "%s: V = %d, rows = %d (rows 1 .. 65535)", fn, V, rows);
  int r = check_lang_list(nullptr, fn, lang_ids_host, n_lang, V);
  if (r != TW_OK) return r;
  DeviceGuard guard(device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // one block: ids [n_lang] | out ids [rows] | out probabilities [rows][n_lang]
  const size_t words = (size_t)n_lang + rows + (size_t)rows * n_lang;
  int* dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), sizeof(int) * words);
  if (e != hipSuccess) return fail(nullptr, TW_ENOMEM, "%s: hipMalloc failed: %s", fn, hipGetErrorString(e));
  int* out_id = dev + n_lang;
  float* out_prob = reinterpret_cast<float*>(out_id + rows);
  e = hipMemcpyAsync(dev, lang_ids_host, sizeof(int) * n_lang, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_lang_detect(logits_dev, V, rows, dev, n_lang, out_id, out_prob_host ? out_prob : nullptr, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_id_host, out_id, sizeof(int) * rows, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && out_prob_host) e = hipMemcpyAsync(out_prob_host, out_prob, sizeof(float) * (size_t)rows * n_lang, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  (void)hipFree(dev);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(nullptr, TW_EHIP, "%s: %s", fn, hipGetErrorString(e));
  return TW_OK;
}

int tw_detect_language(tw_ctx* c, int32_t B, int32_t sot_id, const int32_t* lang_ids_host, int32_t n_lang, int32_t* out_id_host,
                       float* out_prob_host, void* stream) {
  const char* fn = "tw_detect_language";
  if (!c) return TW_EINVAL;
  if (!lang_ids_host || !out_id_host) return fail(c, TW_EINVAL, "%s: null argument", fn);
  TW_ON_DEVICE(c);
  if (B < 1 || B > c->Bmax) return fail(c, TW_EINVAL, "%s: B = %d outside 1 .. max_batch = %d", fn, B, c->Bmax);
  if (sot_id < 0 || sot_id >= c->V) return fail(c, TW_EINVAL, "%s: sot_id %d outside [0, %d)", fn, sot_id, c->V);
  int r = check_lang_list(c, fn, lang_ids_host, n_lang, c->V);
  if (r != TW_OK) return r;
  if (B > c->cross_B) return fail(c, TW_ESTATE, "%s: B=%d but cross K/V holds %d clips", fn, B, c->cross_B);
  hipStream_t st = pick_stream(c, stream);
  const size_t Bm = (size_t)c->Bmax, cap = TW_LANG_MAX + Bm + Bm * TW_LANG_MAX + Bm;
  r = upload_first_use_table(c, c->lang_tab, c->h_lang, cap, true, lang_ids_host, (size_t)n_lang, st);
  if (r != TW_OK) return r;
  const size_t o_id = TW_LANG_MAX, o_prob = o_id + Bm, o_sot = o_prob + Bm * TW_LANG_MAX;
  for (int b = 0; b < B; ++b) c->h_lang[o_sot + b] = sot_id;
  // the launches of tw_decoder_reset + tw_decode_step
  r = reset_state(c, 0, st);
  if (r != TW_OK) return r;
  c->dec_key_bound = c->P;
  HIPCHK(c, hipMemcpyAsync(c->cur_ids, c->h_lang + o_sot, sizeof(int) * B, hipMemcpyHostToDevice, st));
  r = decode_core(c, B, st);
  if (r != TW_OK) return r;
  float* prob_dev = reinterpret_cast<float*>(c->lang_tab + o_prob);
  HIPCHK(c, launch_lang_detect(c->logits, c->V, B, c->lang_tab, n_lang, c->lang_tab + o_id, out_prob_host ? prob_dev : nullptr, st));
  HIPCHK(c, launch_advance(c->stt, 1, st));
  HIPCHK(c, hipMemcpyAsync(c->h_lang + o_id, c->lang_tab + o_id, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  if (out_prob_host)
    HIPCHK(c, hipMemcpyAsync(c->h_lang + o_prob, prob_dev, sizeof(float) * (size_t)B * n_lang, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  memcpy(out_id_host, c->h_lang + o_id, sizeof(int) * B);
  if (out_prob_host) memcpy(out_prob_host, c->h_lang + o_prob, sizeof(float) * (size_t)B * n_lang);
  return TW_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Resampling front end (k_resample.hip): the plan and the prototype taps are host arithmetic in double, so C-ABI users get
// them without Python; the float32 table is uploaded once per (device, sr_in, sr_out) and kept for the process.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kResampleZ = 16;               // zero crossings of the sinc kept on each side, in units of F
constexpr double kResampleBeta = 8.6;        // Kaiser window
constexpr double kResampleRho = 0.945;       // cut-off as a fraction of the narrower Nyquist
constexpr long long kResampleMaxTaps = 1 << 18;   // 1 MiB of float32 on the device

struct ResamplePlan { int L, M, half, taps_per_output; };

double bessel_i0(double x) {                 // power series: sum ((x/2)^k / k!)^2
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

int resample_plan(const char* who, int32_t sr_in, int32_t sr_out, ResamplePlan* p) {
  if (sr_in < 4000 || sr_out < 4000) return fail(nullptr, TW_EINVAL, "%s: sample rates must be >= 4000 Hz (got %d -> %d)", who, sr_in, sr_out);
  long long a = sr_in, b = sr_out;
  while (b) { const long long t = a % b; a = b; b = t; }
  const long long L = sr_out / a, M = sr_in / a, F = std::max(L, M);
  if (L == 1 && M == 1) { *p = {1, 1, 0, 1}; return TW_OK; }      // same rate: the one-tap table {1}, a bit-exact copy
  const long long half = kResampleZ * F;
  if (2 * half + 1 > kResampleMaxTaps)
    return fail(nullptr, TW_EINVAL, "%s: %d -> %d Hz needs a table of %lld taps (L=%lld M=%lld), more than the supported %lld", who, sr_in,
                sr_out, 2 * half + 1, L, M, kResampleMaxTaps);
  *p = {(int)L, (int)M, (int)half, (int)(2 * half / L) + 1};
  return TW_OK;
}

void resample_taps(const ResamplePlan& p, double* h) {
  if (p.half == 0) { h[0] = 1.0; return; }
  const double F = (double)std::max(p.L, p.M), fc = kResampleRho / F, i0b = bessel_i0(kResampleBeta), pi = 3.14159265358979323846;
  for (int j = -p.half; j <= p.half; ++j) {
    const double u = (double)j / (double)p.half, a = pi * fc * (double)j;
    const double sinc = j == 0 ? 1.0 : std::sin(a) / a;
    h[j + p.half] = (double)p.L * fc * sinc * bessel_i0(kResampleBeta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
  }
}

std::mutex g_resample_mu;
std::map<std::tuple<int, int, int>, float*> g_resample_tables;   // (device, sr_in, sr_out) -> float32 [2 half + 1], device

int resample_table(int device, int32_t sr_in, int32_t sr_out, const ResamplePlan& p, const float** out) {
  std::lock_guard<std::mutex> lock(g_resample_mu);
  const auto key = std::make_tuple(device, (int)sr_in, (int)sr_out);
  auto it = g_resample_tables.find(key);
  if (it == g_resample_tables.end()) {
    const size_t n = 2 * (size_t)p.half + 1;
    std::vector<double> h(n);
    resample_taps(p, h.data());
    std::vector<float> hf(h.begin(), h.end());
    float* d = nullptr;
    HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&d), n * sizeof(float)));
    hipError_t e = hipMemcpy(d, hf.data(), n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return fail(nullptr, TW_EHIP, "tw_resample: tap table upload failed: %s", hipGetErrorString(e));
    }
    it = g_resample_tables.emplace(key, d).first;
  }
  *out = it->second;
  return TW_OK;
}

}  // namespace

extern "C" {

int tw_resample_plan(int32_t sr_in, int32_t sr_out, int32_t* L, int32_t* M, int32_t* half, int32_t* taps_per_output) {
  ResamplePlan p;
  const int rc = resample_plan("tw_resample_plan", sr_in, sr_out, &p);
  if (rc != TW_OK) return rc;
  if (L) *L = p.L;
  if (M) *M = p.M;
  if (half) *half = p.half;
  if (taps_per_output) *taps_per_output = p.taps_per_output;
  return TW_OK;
}

int tw_resample_taps(int32_t sr_in, int32_t sr_out, double* out_host, int32_t n) {
  if (!out_host) return fail(nullptr, TW_EINVAL, "tw_resample_taps: null argument");
  ResamplePlan p;
  const int rc = resample_plan("tw_resample_taps", sr_in, sr_out, &p);
  if (rc != TW_OK) return rc;
  if (n != 2 * p.half + 1) return fail(nullptr, TW_EINVAL, "tw_resample_taps: n=%d, the %d -> %d Hz table has %d taps", n, sr_in, sr_out, 2 * p.half + 1);
  resample_taps(p, out_host);
  return TW_OK;
}

int tw_resample(int32_t device, const void* in_dev, int32_t in_fmt, int32_t channels, int64_t in_stride_frames,
                const int64_t* in_first_host, const int32_t* in_count_host, int32_t sr_in, int32_t sr_out,
                const int64_t* out_first_host, int32_t n_out, float* out_dev, int64_t out_stride, int32_t B, void* stream) {
  if (!in_dev || !in_first_host || !in_count_host || !out_first_host || !out_dev) return fail(nullptr, TW_EINVAL, "tw_resample: null argument");
  if (in_fmt != TW_PCM_F32 && in_fmt != TW_PCM_S16) return fail(nullptr, TW_EINVAL, "tw_resample: in_fmt %d is not TW_PCM_F32 / TW_PCM_S16", in_fmt);
  if (B < 1 || B > 64) return fail(nullptr, TW_EINVAL, "tw_resample: B=%d outside [1,64]", B);
  if (channels < 1 || channels > 8) return fail(nullptr, TW_EINVAL, "tw_resample: channels=%d outside [1,8]", channels);
  if (n_out < 1) return fail(nullptr, TW_EINVAL, "tw_resample: n_out=%d, nothing to produce", n_out);
  if (out_stride < n_out || in_stride_frames < 0) return fail(nullptr, TW_EINVAL, "tw_resample: a row stride is shorter than the row");
  if (reinterpret_cast<uintptr_t>(in_dev) & (in_fmt == TW_PCM_S16 ? 1 : 3)) return fail(nullptr, TW_EINVAL, "tw_resample: in_dev is not aligned to its sample type");
  ResamplePlan p;
  int rc = resample_plan("tw_resample", sr_in, sr_out, &p);
  if (rc != TW_OK) return rc;
  ResampleArgs a{};
  for (int b = 0; b < B; ++b) {
    if (in_count_host[b] < 0 || in_count_host[b] > in_stride_frames || out_first_host[b] < 0 ||
        in_first_host[b] < -((int64_t)1 << 40) || in_first_host[b] > ((int64_t)1 << 40) || out_first_host[b] > ((int64_t)1 << 40))
      return fail(nullptr, TW_EINVAL, "tw_resample: row %d: in_count %d (stride %lld frames), in_first %lld, out_first %lld", b,
                  in_count_host[b], (long long)in_stride_frames, (long long)in_first_host[b], (long long)out_first_host[b]);
    a.rows.in_first[b] = in_first_host[b];
    a.rows.in_count[b] = in_count_host[b];
    a.rows.out_first[b] = out_first_host[b];
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, TW_EHIP, "no HIP device available (the MI355X path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, TW_EINVAL, "device %d out of range", device);
  DeviceGuard guard(device);
  const float* taps = nullptr;
  rc = resample_table(device, sr_in, sr_out, p, &taps);
  if (rc != TW_OK) return rc;
  a.in = in_dev; a.s16 = in_fmt == TW_PCM_S16; a.channels = channels; a.in_stride_frames = in_stride_frames;
  a.taps = taps; a.L = p.L; a.M = p.M; a.half = p.half;
  a.out = out_dev; a.out_stride = out_stride; a.n_out = n_out; a.B = B;
  hipError_t e = launch_resample(a, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, TW_EHIP, "resample_kernel: %s", hipGetErrorString(e));
  return TW_OK;
}

int tw_stream_create_masked(int32_t device, const uint32_t* cu_mask, int32_t n_words, void** out_stream) {
  if (!cu_mask || n_words < 1 || !out_stream) return TW_EINVAL;
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)n_words, cu_mask);
  if (e != hipSuccess) { g_create_error = std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e); return TW_EHIP; }
  *out_stream = st;
  return TW_OK;
}

int tw_stream_destroy(void* stream) {
  if (!stream) return TW_OK;
  (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
  return hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? TW_OK : TW_EHIP;
}

int tw_stream_synchronize(void* stream) {
  return hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? TW_OK : TW_EHIP;
}

int tw_event_create(int32_t device, void** out_event) {
  if (!out_event) return TW_EINVAL;
  DeviceGuard guard(device);
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return TW_EHIP;
  *out_event = ev;
  return TW_OK;
}

int tw_event_destroy(void* event) {
  if (!event) return TW_OK;
  return hipEventDestroy(reinterpret_cast<hipEvent_t>(event)) == hipSuccess ? TW_OK : TW_EHIP;
}

int tw_event_record(void* event, void* stream) {
  return hipEventRecord(reinterpret_cast<hipEvent_t>(event), reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? TW_OK : TW_EHIP;
}

int tw_stream_wait_event(void* stream, void* event) {
  return hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<hipEvent_t>(event), 0) == hipSuccess ? TW_OK : TW_EHIP;
}

}  // extern "C"
