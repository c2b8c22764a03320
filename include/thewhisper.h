/*
 * thewhisper.h - C ABI of libthewhisper_gfx950.so, the MI355X (gfx950 / CDNA4) Whisper hot path.
 *
 * The reference (TheStageAI/TheWhisper) has NO C ABI / FFI for this path: its NVIDIA backend hands
 * the whole computation to a Python model object (Hugging Face `WhisperForConditionalGeneration`, or
 * the closed TensorRT wheel) under `ASRPipeline` (R:thestage_speechkit/nvidia/asr_pipeline.py:47-60),
 * and its Apple backend swaps encoder/decoder modules under the same object
 * (R:thestage_speechkit/apple/model.py:601-614).  Each entry point below therefore cites the
 * Python-level interface it replaces (R: = /root/reference, HF: = transformers 5.15.0).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0 on success
 *    and a negative TW_E* code on failure; tw_last_error() returns a human-readable message.
 *  - "dev" pointers are HIP device pointers owned by the caller (torch); the library never frees
 *    them and never retains them after the call returns, except nothing: weights are COPIED
 *    (converted / repacked) into the context at tw_load_weight time.
 *  - "host" pointers are ordinary host memory.  Calls that return host data synchronise the
 *    stream; all other calls only enqueue work on `stream` (a hipStream_t passed as void*; pass
 *    torch's current stream so ordering with torch ops is automatic; NULL = default stream).
 *  - A context is bound to one device, owns its workspace / KV arenas (allocated in tw_create, freed
 *    in tw_destroy) and is NOT thread-safe: one context per (GPU, worker thread).  Every call makes the
 *    context's device current for its duration and restores the calling thread's device on return.
 *  - Batch entries ("streams") of one call occupy slots 0..B-1 of the context, B <= max_batch.
 */
#ifndef THEWHISPER_H
#define THEWHISPER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TW_VERSION_STRING "thewhisper-gfx950 0.1.0"

/* element types of caller buffers and of the context's compute mode */
enum { TW_F32 = 0, TW_BF16 = 1, TW_F16 = 2,
       TW_BF16_MXFP8 = 3, /* context dtype only: bf16 activations / encoder, decoder projection weights as MXFP8 (OCP e4m3 +
                            one power-of-two scale per 32 values) AND the activations quantised the same way in registers, on
                            v_mfma_scale_f32_16x16x128_f8f6f4 ("W8A8"); fp8 cross-attention K / V caches; BASELINE config 5 */
       TW_BF16_W8A16 = 4  /* context dtype only: the same MXFP8 weights and fp8 cross K / V caches, but the weight fragments are
                            widened to bf16 in registers and contracted with the UNQUANTISED bf16 activations on the bf16 MFMA
                            ("W8A16": same bytes from HBM, no activation-quantisation error); up to 64 streams */ };

/* error codes */
enum {
  TW_OK = 0,
  TW_EINVAL = -1,   /* bad argument / unsupported configuration */
  TW_EHIP = -2,     /* HIP runtime error (message has the hipError string) */
  TW_ESTATE = -3,   /* call order violated (e.g. decode before encode / weights not finalized) */
  TW_ENOMEM = -4,
  TW_ENAME = -5     /* unknown weight name or shape mismatch */
};

#define TW_MAX_ALIGN_HEADS 32

typedef struct tw_ctx tw_ctx;

/* Model + capacity description.  Mirrors the fields of HF `WhisperConfig` that the hot path uses
 * (HF:models/whisper/configuration_whisper.py) plus the per-context capacities. */
typedef struct tw_config {
  int32_t d_model;
  int32_t enc_layers;
  int32_t dec_layers;
  int32_t heads;                 /* head_dim = d_model / heads must be 64 */
  int32_t ffn;
  int32_t vocab;
  int32_t n_mels;
  int32_t source_positions;      /* T: encoder frames per chunk = 50 * chunk_seconds (<= 1500).  When
                                    < 1500 the 1500-row positional table is linearly interpolated at
                                    load time exactly like patch_hf_model
                                    (R:thestage_speechkit/nvidia/asr_pipeline.py:15-27). */
  int32_t target_positions;      /* decoder positions, 448 */
  int32_t max_batch;             /* concurrent streams per call: 1..64 (1..16 with TW_BF16_MXFP8) */
  int32_t dtype;                 /* TW_BF16 (production), TW_F16 (the reference's streaming default dtype,
                                    R:thestage_speechkit/streaming/streaming_pipeline.py:369-370: same MFMA rate, 10 mantissa bits,
                                    activations saturate at 65504 as HF clamps its float16 hidden states), TW_F32 (strict-parity
                                    mode), TW_BF16_MXFP8 / TW_BF16_W8A16 (fp8 decoder weights) */
  int32_t n_align_heads;         /* alignment heads for word timestamps (generation_config.alignment_heads) */
  int32_t align_heads[2 * TW_MAX_ALIGN_HEADS]; /* (layer, head) pairs */
  int32_t device;                /* HIP device ordinal */
  int32_t use_graph;             /* 1: replay the decode step from a captured hipGraph */
} tw_config;

/* Options of one greedy decode (A9/A10).  Mirrors what HF's generate derives from
 * generation_config + the three Whisper logits processors
 * (HF:models/whisper/generation_whisper.py:1774-1812, HF:generation/logits_process.py:1816-2047).
 * Every tw_generate_* call and tw_score_tokens check them alike and answer TW_EINVAL to: a list count that is negative or above its
 * capacity (64 begin-suppress ids, 1024 suppress ids), a positive count with a NULL list, pad_id or eos_id outside the vocabulary. */
typedef struct tw_greedy_opts {
  int32_t eos_id;
  int32_t pad_id;
  int32_t max_new_tokens;
  int32_t min_new_tokens;        /* MinNewTokensLength: eos masked until this many new tokens */
  int32_t max_length;            /* prompt + new tokens cap (generation_config.max_length) */
  int32_t timestamps;            /* 1: apply WhisperTimeStampLogitsProcessor */
  int32_t no_timestamps_id;      /* timestamp_begin = no_timestamps_id + 1 */
  int32_t max_initial_timestamp_index; /* < 0: unset */
  int32_t n_begin_suppress;
  const int32_t* begin_suppress; /* host */
  int32_t n_suppress;
  const int32_t* suppress;       /* host */
  int32_t want_alignment;        /* 1: record alignment-head cross-attention rows for tw_token_timestamps */
  int32_t n_forced;              /* the last n_forced tokens of every prompt row are FORCED OUTPUT, not prompt: they count as generated
                                    (begin index = n_prompt - n_forced: max_new_tokens, min_new_tokens and the timestamp grammar see
                                    them as tokens the loop produced), and positions 0 .. n_prompt-2 are processed by a batched
                                    prefill (rows = streams x positions per launch) instead of one step each.  What it is for:
                                    SURVEY.md section 8f-3 - a streaming backend re-decodes every 0.5 s a buffer most of whose text
                                    it emitted a moment ago (R:thestage_speechkit/streaming/streaming_pipeline.py:770-796) and may
                                    force that text and decode only the tail (thewhisper_amd/streaming.py, opt-in).  0 = off. */
  int32_t n_draft;               /* the last n_draft tokens of every prompt row are a DRAFT of the output (exact form):
                                    GUESSES, e.g. what the previous 0.5 s tick of the same stream produced
                                    (R:thestage_speechkit/streaming/streaming_pipeline.py:388-435 decodes the rolling buffer from scratch
                                    every tick, :770-796).  The call returns exactly what it returns with the same prompt WITHOUT
                                    them - same ids, same alignment rows - however good the guesses are: prompt and draft are run
                                    through the decoder in launches of up to 64 rows (streams x consecutive positions) WITH the logits
                                    and the logits processors of every row; the draft is accepted up to the first position where
                                    some stream's arg-max differs from its guess, that arg-max becomes the token there, the rest of
                                    the draft is offered again behind it, and the one-token-per-step loop takes over where nothing
                                    more is confirmed.  A draft holds no <eos> (TW_EINVAL), so a stream whose arg-max is <eos> always
                                    ends its round; whatever stands behind that position in ANY stream's draft is then dropped - no
                                    further round is offered once a stream has finished - and the one-token loop goes on from there:
                                    the finished stream receives pad_id, the others are decoded step by step, out_len is set by the last
                                    <eos> as in the plain call.  Guesses that run on behind a stream's end (a previous tick that was
                                    longer than this one) therefore cost time, never a token.
                                    Sound because a row's result does not depend on the other rows of its launch
                                    (one reduction order for every launch width, k_decode.hip).  Begin index = n_prompt - n_draft.
                                    Not together with n_forced.  0 = off.  tw_last_draft reports what was accepted. */
} tw_greedy_opts;

const char* tw_version(void);
/* ctx may be NULL: returns the message of the last failed tw_create on this thread. */
const char* tw_last_error(const tw_ctx* ctx);

/* Replaces: model construction under ASRPipeline.__init__
 * (R:thestage_speechkit/nvidia/asr_pipeline.py:47-60). */
int tw_create(const tw_config* cfg, tw_ctx** out);
int tw_destroy(tw_ctx* ctx);
/* A second context of the SAME model on the same device that shares `src`'s finalized weights (no copy: `src` owns them and must be
 * destroyed after the sibling) and has its own workspace, K/V arenas (for `max_batch` streams), graphs and timing events.  What it
 * is for: two stages of a serving pipeline on one GPU at the same time - the encoder stage of new chunks on a CU-masked stream
 * while the decode loop of the current pass runs (a context is not thread-safe, two contexts are independent).  No reference
 * counterpart (one pipeline object, one request at a time: R:examples/server.py:22-115). */
int tw_create_sibling(const tw_ctx* src, int32_t max_batch, tw_ctx** out);

/* Replaces: `from_pretrained` weight materialisation (R:thestage_speechkit/nvidia/asr_pipeline.py:58-60).
 * `name` is the HF state_dict key (layout table in SURVEY.md section 8b), `dev_ptr` a contiguous device tensor
 * of element type `dtype` (TW_F32/TW_BF16/TW_F16) and shape `shape[ndim]`.  The tensor is converted to
 * the context dtype and copied/repacked; the caller may free it afterwards. */
int tw_load_weight(tw_ctx* ctx, const char* name, const void* dev_ptr, int32_t dtype, int32_t ndim,
                   const int64_t* shape, void* stream);
/* Checks that every tensor arrived, interpolates the encoder positions (A0) and folds each decoder pre-LayerNorm
 * into the projection that consumes it (W <- W*gain plus two per-row vectors).  Call exactly once. */
int tw_finalize_weights(tw_ctx* ctx, void* stream);

/* A1.  Replaces: WhisperFeatureExtractor._torch_extract_fbank_features
 * (HF:models/whisper/feature_extraction_whisper.py:135-168) as called from the ASR pipeline
 * (HF:pipelines/automatic_speech_recognition.py:67-72).
 * pcm_dev: float32 [B, pcm_stride] mono 16 kHz; n_valid_host[b] (may be NULL = n_samples) samples
 * are real, the rest up to n_samples is treated as zero padding; out_dev: [B, n_mels, n_samples/160]
 * of element type out_dtype (TW_F32 or the context dtype). */
int tw_logmel(tw_ctx* ctx, const float* pcm_dev, int64_t pcm_stride, const int32_t* n_valid_host, int32_t B,
              int32_t n_samples, void* out_dev, int32_t out_dtype, void* stream);

/* A2-A4.  Replaces: WhisperEncoder.forward (HF:models/whisper/modeling_whisper.py:540-646).
 * mel_dev: [B, n_mels, 2T] of mel_dtype (TW_F32 / TW_BF16 / TW_F16).  The encoder output is kept inside the context (slots
 * 0..B-1); if out_hidden_dev != NULL it is also written there as [B, T, d_model] in out_dtype (TW_F32 / TW_BF16). */
int tw_encode(tw_ctx* ctx, const void* mel_dev, int32_t mel_dtype, int32_t B, void* out_hidden_dev,
              int32_t out_dtype, void* stream);

/* Test instrument: tw_encode with taps.  Runs exactly the launches of tw_encode and copies named intermediate buffers of encoder
 * layer `layer` into caller-supplied DEVICE buffers, each right after the launch that produced it (hipMemcpyAsync device-to-device
 * on the call's stream).  A NULL member is not copied; with every member NULL (or taps == NULL) the call is tw_encode.  Every
 * copy takes the WHOLE workspace buffer, sized for max_batch clips, not just the B clips of the call, so that a caller can see
 * whether a launch wrote past its rows.  Element type: the context dtype, except the two float32 statistics buffers.  With
 * Bm = max_batch, T = source_positions, d = d_model, H = heads, F = ffn, Tp = T rounded up to 64:
 *   h1          [Bm, 2T+2, d]   conv1 + GELU, token-major, rows 0 and 2T+1 of every clip are the zero padding of conv2
 *   xa_in       [Bm*T, d]       the layer's input (layer 0: conv2 + GELU + positions)
 *   ln_stats_a  [Bm*T, d/32, 2] float32 (sum, sum of squares) per 32-column block of xa_in as stored; written only in contexts
 *                               that fold the encoder's LayerNorms into the GEMMs (d_model % 64 == 0 and <= 1280)
 *   q, k        [Bm, H, T, 64]  q carries the 1/8 scale
 *   vt          [Bm, H, 64, Tp] V transposed, keys [T, Tp) zero
 *   attn        [Bm*T, d]       softmax(q k^T) v, heads merged
 *   xb          [Bm*T, d]       xa_in + out-projection
 *   ln_stats_b  [Bm*T, d/32, 2] float32, of xb
 *   ffnh        [Bm*T, F]       GELU(fc1)
 *   xa_out      [Bm*T, d]       xb + fc2: the layer's output
 *   enc_out     [Bm*T, d]       the encoder output slots after the final LayerNorm */
typedef struct tw_encode_taps {
  int32_t layer;
  void *h1, *xa_in, *q, *k, *vt, *attn, *xb, *ffnh, *xa_out, *enc_out;
  float *ln_stats_a, *ln_stats_b;
} tw_encode_taps;
int tw_encode_tapped(tw_ctx* ctx, const void* mel_dev, int32_t mel_dtype, int32_t B, void* out_hidden_dev,
                     int32_t out_dtype, const tw_encode_taps* taps, void* stream);

/* Host only, no GPU and no context needed: which kernel the encoder's launches take for a shape, so that a test can prove which
 * code it reached.  tw_gemm_plan: dtype = TW_F32 / TW_BF16 / TW_F16, mode = 0 for a row-major output, 2 for the encoder's fused
 * QKV projection, 3 for the cross K/V projection; C[M, N] = A[M, K] W[N, K]^T; *kernel = 1 (both operands through LDS, bm x 64
 * tiles) or 2 (weights straight to registers, bm x 256 tiles), *bm = the tile height.  tw_enc_attention_plan: B streams of H
 * heads and T frames; *queries_per_block = 64 or 128, *xcd = 1 when heads are pinned to XCDs.  Any output pointer may be NULL. */
int tw_gemm_plan(int32_t dtype, int32_t mode, int32_t M, int32_t N, int32_t K, int32_t* kernel, int32_t* bm);
int tw_enc_attention_plan(int32_t dtype, int32_t B, int32_t H, int32_t T, int32_t* queries_per_block, int32_t* xcd);

/* A5.  Replaces: the lazy cross-attention K/V projection + EncoderDecoderCache.is_updated
 * (HF:models/whisper/modeling_whisper.py:312-335).  Projects the context's encoder output of slots
 * 0..B-1 into the per-layer cross K/V arenas, once per chunk. */
int tw_cross_kv(tw_ctx* ctx, int32_t B, void* stream);

/* The same two stages for slots slot0 .. slot0+B-1 of the context, leaving the other slots as they are: a serving pass is
 * then assembled from several groups of chunks (the ones that need a further Whisper seek iteration first, late arrivals
 * while those are being encoded), and ONE tw_generate_greedy runs over all of them.  There is no reference counterpart
 * (HF's generate() encodes a fixed batch, HF:models/whisper/generation_whisper.py:785-903); results per slot are
 * independent of the grouping.  tw_encode / tw_cross_kv are the slot0 = 0 forms and reset the number of filled slots. */
int tw_encode_at(tw_ctx* ctx, const void* mel_dev, int32_t mel_dtype, int32_t B, int32_t slot0, void* stream);
int tw_cross_kv_at(tw_ctx* ctx, int32_t B, int32_t slot0, void* stream);

/* Cross K/V of slots src_slot0 .. src_slot0+B-1 of `src` become slots dst_slot0 .. dst_slot0+B-1 of `dst` (device-to-device copies
 * on `stream`; both contexts: same model dimensions, same source_positions, same dtype, same device; dst_slot0 must be the
 * number of slots `dst` holds, like tw_cross_kv_at).  `src_stream` = the stream `src`'s encoder stage was enqueued on (NULL = its
 * default): the copies are ordered after everything enqueued there so far, and whatever is enqueued there next after the copies
 * (so the source may refill the slots at once).  The caller must not run another call on `src` concurrently with this one.  What it is for: a serving loop encodes the chunks that ARRIVE while a pass is
 * decoding on a second context of the same weights (its own workspace and arenas, a CU-masked stream), and the next pass adopts
 * them - their encoder stage is then hidden under the previous pass's decode loop (thewhisper_amd/serving.py).  No reference
 * counterpart (R:examples/server.py:22-115 processes one request at a time).  Results are the ones tw_encode_at + tw_cross_kv_at
 * on `dst` would have produced: same kernels, same weights. */
int tw_adopt_cross_kv(tw_ctx* dst, int32_t dst_slot0, tw_ctx* src, int32_t src_slot0, int32_t B, void* stream, void* src_stream);

/* A6-A8.  Replaces: WhisperDecoder.forward + proj_out for ONE new token per stream
 * (HF:models/whisper/modeling_whisper.py:649-795, :1080).  tw_decoder_reset rewinds the self-attention
 * cache to position 0.  ids_host: int32 [B].  logits_dev: float32 [B, vocab] or NULL. */
int tw_decoder_reset(tw_ctx* ctx, int32_t B, void* stream);
int tw_decode_step(tw_ctx* ctx, int32_t B, const int32_t* ids_host, float* logits_dev, void* stream);

/* A9+A10.  Replaces: GenerationMixin._sample (HF:generation/utils.py:2783-2946) for num_beams=1,
 * do_sample=False with Whisper's logits processors, as invoked by
 * WhisperGenerationMixin.generate_with_fallback (HF:models/whisper/generation_whisper.py:1027).
 * prompt_host: int32 [B, n_prompt]; out_ids_host: int32 [B, max_length] receives prompt + generated
 * tokens padded with pad_id; out_len_host[0] = common sequence length (HF pads finished rows).
 * Requires tw_encode + tw_cross_kv for the same B. */
int tw_generate_greedy(tw_ctx* ctx, int32_t B, const int32_t* prompt_host, int32_t n_prompt,
                       const tw_greedy_opts* opts, int32_t* out_ids_host, int32_t* out_len_host, void* stream);

/* tw_generate_greedy with a per-stream sequence bias ("hotword boosting").  Replaces: SequenceBiasLogitsProcessor
 * (HF:generation/logits_process.py:1211-1319), which HF's generate builds at the head of its processor list
 * (HF:generation/utils.py:1154-1155) so that Whisper's own processors see the biased scores.  HF takes one list per generate call; here
 * every row (stream) of the call has its own, applied on the device inside the step.
 *
 * THE RULE.  Row b consumes position p and produces the token at p + 1.  h = the row's ids at positions 0 .. p, n = p + 1 of them: prompt,
 * forced tokens and draft tokens included, as HF's input_ids.  x = the row's float32 logits as the model produced them.  A sequence s =
 * t[0 .. L-1] with bias beta (finite float32) of row b is ACTIVE iff
 *     L == 1,   or   L <= n  and  h[n - (L-1) + j] == t[j] for j = 0 .. L-2.
 * (L <= n is HF's `len(sequence_ids) > input_ids.shape[1]: continue`: a sequence whose L-1 prefix is exactly the whole history has
 * L == n + 1 and is NOT applied.)  For every id v that is the last token of at least one active sequence of the row,
 *     total(v) = the float32 sum, starting from 0.0f, of the biases of the active sequences ending in v: the row's length-1 sequence for
 *                v first (if it has one), then the longer ones in the order the caller listed them (HF: zeros + length_1_bias, then
 *                `+=` in dict order),
 *     x'[v] = x[v] + total(v)     one float32 add, HF's `scores + bias`;
 * every other logit keeps its bits.  Everything else in the step reads x' and is otherwise unchanged, bit for bit: the suppress lists,
 * begin-suppress, the min_new_tokens <eos> mask, the timestamp grammar, "the timestamp mass beats every text token", the lowest-id
 * arg-max.  A masked id stays masked (-inf plus a finite value is -inf).  A row without sequences produces the unbiased call's tokens
 * bit for bit, whatever the other rows carry; a row's result does not depend on its slot or on its batch-mates.
 *
 * bopts == NULL or n_seq == 0: the call IS tw_generate_greedy, launch for launch.  Otherwise a step issues one launch more (one
 * workgroup per row; no atomics, no cross-thread sum: the order above is the order of the additions), captured step graphs are kept
 * apart from the unbiased call's, n_forced and n_draft are honoured (the rows-mode launches of a draft's verification are biased the
 * same way, so the result is the biased plain call's: same ids, same alignment rows), and tw_last_draft, tw_last_timings,
 * want_alignment and tw_token_timestamps behave as after tw_generate_greedy.  The tables live in context-owned device memory, allocated
 * by the first biased call of a context (a sibling owns its own) and freed by tw_destroy.
 *
 * TW_EINVAL in addition to tw_generate_greedy's, all before any work is enqueued (the context stays usable): row_off / seq_off that do
 * not start at 0 or decrease, row_off[B] != n_seq, seq_off that does not strictly increase (an empty sequence), a sequence longer than
 * TW_BIAS_MAX_SEQ_LEN, a token outside [0, vocab), a NaN or infinite bias, the same token sequence twice in one row, more than
 * TW_BIAS_MAX_SEQS sequences or TW_BIAS_MAX_TOKENS tokens in the call, B > 64.  tw_generate_sample* take no bias. */
#define TW_BIAS_MAX_SEQS 16384      /* sequences per call, all rows together */
#define TW_BIAS_MAX_TOKENS 65536    /* tokens per call */
#define TW_BIAS_MAX_SEQ_LEN 32      /* tokens per sequence */
typedef struct tw_bias_opts {
  int32_t        n_seq;     /* sequences of all rows together */
  const int32_t* row_off;   /* host [B + 1]: row b owns sequences row_off[b] .. row_off[b+1]-1; a row may own none */
  const int32_t* seq_off;   /* host [n_seq + 1]: tokens of sequence i = tokens[seq_off[i] .. seq_off[i+1]) */
  const int32_t* tokens;    /* host */
  const float*   bias;      /* host [n_seq] */
} tw_bias_opts;
int tw_generate_greedy_biased(tw_ctx* ctx, int32_t B, const int32_t* prompt_host, int32_t n_prompt, const tw_greedy_opts* opts,
                              const tw_bias_opts* bopts, int32_t* out_ids_host, int32_t* out_len_host, void* stream);

/* tw_generate_greedy (or _biased) with a per-stream repetition penalty and a per-stream no-repeat n-gram size.  Replaces:
 * RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor (HF:generation/logits_process.py), which HF's generate builds in the
 * order sequence bias, repetition penalty, no-repeat n-gram (HF:generation/utils.py:1154-1183), all three ahead of Whisper's own
 * processors (appended at :1293).  HF takes one value per generate call; here every row (stream) of the call has its own.
 *
 * THE RULE.  Row b consumes position p and produces the token at p + 1.  h = the row's ids at positions 0 .. p, n = p + 1 of them: prompt,
 * forced tokens and draft tokens included, as HF's input_ids.  x = the row's float32 logits after the row's sequence bias, if it has one.
 *   1. Penalty.  r = penalty[b], a finite float32 > 0; 1.0f = off.  S = { h[i] : penalty_ignore <= i < n } (penalty_ignore is HF's
 *      prompt_ignore_length; 0 is what HF's generate uses).  For every DISTINCT id v of S
 *          x'[v] = x[v] < 0 ? x[v] * r : x[v] / r
 *      one float32 multiply or one correctly rounded float32 division (not a multiply by a reciprocal), from the ORIGINAL x[v]: an id
 *      that occurs twice is penalised once (HF gathers the original score for every occurrence and scatters equal values).  +0, -0 and
 *      -inf follow from the expression as written (+0 and -0 are divided; -inf stays -inf).
 *   2. No-repeat n-gram.  N = no_repeat_ngram[b]; 0 = off.  Nothing happens while n < N.  Otherwise, for every i in 0 .. n - N with
 *          h[i + j] == h[n - N + 1 + j]  for j = 0 .. N - 2
 *      x'[h[i + N - 1]] = -inf.  The whole history is read (penalty_ignore does not apply); N == 1 bans every id of the history.
 *      1 and 2 commute (-inf * r is -inf).
 *   3. Everything else in the step reads x' and keeps its bits: the suppress lists, begin-suppress, the min_new_tokens <eos> mask, the
 *      timestamp grammar, "the timestamp mass beats every text token", the lowest-id arg-max.  The sampler masks an id by treating its
 *      logit as -inf, so a banned id IS a masked id, and a row in which everything is masked or banned returns id 0.
 * A row with r == 1 and N == 0 produces the plain call's tokens bit for bit, whatever the other rows set; a row's result does not depend
 * on its slot or on its batch-mates.  Rows still consuming their prompt and finished rows are left alone.
 *
 * ropts == NULL, or every row off: the call IS tw_generate_greedy (tw_generate_greedy_biased with bopts), launch for launch.  Otherwise a
 * step issues one launch more (one workgroup per row, behind the bias launch and in front of the sampler; no atomics, no store whose
 * value depends on the order of the threads), captured step graphs are kept apart from the other calls' (repeat alone and bias + repeat
 * each have their own), n_forced and n_draft are honoured (the rows-mode launches of a draft's verification are processed the same way,
 * so the result is the processed plain call's: same ids, same alignment rows), and tw_last_draft, tw_last_timings, want_alignment and
 * tw_token_timestamps behave as after tw_generate_greedy.  The per-row table lives in context-owned device memory, allocated by the first
 * call of a context that uses it (a sibling owns its own) and freed by tw_destroy.
 *
 * TW_EINVAL in addition to tw_generate_greedy(_biased)'s, all before any work is enqueued (the context stays usable): a penalty that is
 * NaN, infinite or <= 0; N < 0 or N > target_positions; penalty_ignore < 0; B > 64.  tw_generate_sample*, tw_generate_greedy_ragged and
 * tw_score_tokens take no repeat options. */
typedef struct tw_repeat_opts {
  const float*   penalty;          /* host [B]; 1.0f = off; NULL = off for every row */
  const int32_t* no_repeat_ngram;  /* host [B]; 0 = off; NULL = off for every row */
  int32_t        penalty_ignore;   /* HF's prompt_ignore_length; 0 = HF generate's */
} tw_repeat_opts;
int tw_generate_greedy_repeat(tw_ctx* ctx, int32_t B, const int32_t* prompt_host, int32_t n_prompt, const tw_greedy_opts* opts,
                              const tw_bias_opts* bopts /* may be NULL */, const tw_repeat_opts* ropts,
                              int32_t* out_ids_host, int32_t* out_len_host, void* stream);
/* Parity access, context-free like tw_vad_energy: steps 1 and 2 of the rule above on caller-provided data.  Row r of logits_dev (device,
 * float32 [rows, V], edited in place) is processed with the history hist_host[r * ld .. r * ld + n_hist_host[r]) and ropts->penalty[r],
 * ropts->no_repeat_ngram[r].  The call returns after the stream has been synchronised.  TW_EINVAL: the refusals above (with
 * target_positions = 512, the history one launch holds), rows outside 1 .. 64, ld > 512, n_hist outside [0, ld], a history id outside
 * [0, V), a null pointer. */
int tw_repeat_logits(int32_t device, float* logits_dev, int32_t V, int32_t rows, const int32_t* hist_host, int32_t ld,
                     const int32_t* n_hist_host, const tw_repeat_opts* ropts, void* stream);

/* Language detection on the device (k_decode.hip: lang_detect_kernel): HF's detect_language (HF:models/whisper/generation_whisper.py:1610-1683)
 * masks every non-language logit of the step at <|startoftranscript|> and takes the arg-max.  Here the kernel reads the n_lang listed
 * logits only and nothing of the [rows, V] logits is copied back.
 *
 * THE RULE for row r and the listed ids (any order, not necessarily contiguous), x_j = logits[r][ids[j]]:
 *   a NaN counts as -inf;  m = max_j x_j;
 *   id = the SMALLEST TOKEN ID among the j with x_j == m (not the smallest list index): torch.argmax of HF's masked row - the first
 *     occurrence over the vocabulary.  Logits outside the list never matter, however large;
 *   p_j = exp(x_j - m) / s in float32, s = the float32 sum of the numerators in an order that depends on n_lang only - never on the
 *     number of rows or on the row's index: a row's 32-bit patterns are the same alone and in a batch of 64;
 *   m == -inf (nothing finite in the list): id = the smallest listed id and every p_j = 0.0f.  (A deviation: HF answers id 0 there.)
 * One workgroup per row, no atomics.
 *
 * TW_EINVAL for both entries, before anything is enqueued (a context stays usable): a NULL logits / id-list / out_id pointer, n_lang
 * outside 1 .. TW_LANG_MAX, a listed id (tw_detect_language: or sot_id) outside [0, V), a duplicate id, rows (B) below 1 or above what
 * the call can hold (tw_language_logits: 65535; tw_detect_language: max_batch).  out_prob_host may be NULL: only the ids come back. */
#define TW_LANG_MAX 128
/* context-free, like tw_repeat_logits: the kernel on caller-supplied logits (device, float32 [rows, V], only read).  Test instrument and
 * building block.  Returns after the stream has been synchronised. */
int tw_language_logits(int32_t device, const float* logits_dev, int32_t V, int32_t rows, const int32_t* lang_ids_host, int32_t n_lang,
                       int32_t* out_id_host, float* out_prob_host /* [rows, n_lang] or NULL */, void* stream);
/* Rows 0 .. B-1 of the context's cross K/V (tw_encode + tw_cross_kv for at least B rows, else TW_ESTATE, as tw_decode_step): rewinds the
 * decoder (the launches of tw_decoder_reset), runs ONE step on sot_id for every row (the launches of tw_decode_step) and applies the
 * kernel to that step's logits.  Copies back B ints and, with out_prob_host, B * n_lang floats.  The id list goes to context-owned device
 * memory allocated by the context's first call (tw_destroy frees it; a sibling owns its own).  Leaves the decoder at position 1, like a
 * tw_decode_step; every tw_generate_* call rewinds the decoder, so a following decode is unaffected.  It OVERWRITES the alignment rows
 * and the sampler state of a previous decode: the call belongs in front of the generate call of a pass, never between a generate call
 * and its tw_token_timestamps. */
int tw_detect_language(tw_ctx* ctx, int32_t B, int32_t sot_id, const int32_t* lang_ids_host, int32_t n_lang,
                       int32_t* out_id_host, float* out_prob_host /* [B, n_lang] or NULL */, void* stream);

/* tw_generate_greedy for rows whose prompts differ in length ("ragged prompts"): the batch is LEFT-padded to one length n_prompt, as HF
 * batches Whisper's previous-text prompts (HF:models/whisper/generation_whisper.py:1709-1772 pads decoder_input_ids on the left and passes
 * decoder_attention_mask = ids != pad), and n_pad_host[b] says how many leading entries of row b are padding.
 *
 * THE RULE.  Row b's first n_pad[b] prompt entries are padding: their token values (any valid id) are ignored and returned as given.
 * Row b at absolute position p >= n_pad[b] is at ROW POSITION q = p - n_pad[b]: it takes pos_emb[q], its self-attention K / V go to cache
 * slot q, and it attends slots 0 .. q.  At p < n_pad[b] the row idles: it is treated as row position 0 - it writes slot 0, which the real
 * position 0 overwrites later, and attends that one key - and nothing ever reads what it computes.  Everything else keeps ABSOLUTE
 * positions: the sequence buffer, the begin index (n_prompt, common to all rows), the suppress lists, begin-suppress, the min_new_tokens
 * <eos> mask, the timestamp grammar (it reads history from n_prompt on only), the alignment rows (recorded at absolute p, so
 * tw_token_timestamps and tw_get_alignment work unchanged), out_len_host, tw_last_timings and the step count.
 *
 * CONSEQUENCE.  Row b's generated ids and its alignment rows at p >= n_prompt are bit for bit what tw_generate_greedy produces for that
 * row ALONE when it is given the row's n_prompt - n_pad[b] real tokens as its prompt, the same max_new_tokens and min_new_tokens, and
 * max_length - n_pad[b]: per row every kernel sees exactly the data layout of the alone call, and the self-attention's result does not
 * depend on the 64-key bucket the host picks for a step.  A row's result does not depend on its slot, its batch-mates or their padding.
 * This is NOT HF's arithmetic for a padded batch: HF's generate builds no decoder position ids from the mask, so a padded row keeps
 * absolute positions there and its result depends on how long its batch-mates' prompts are ("Ragged decoder prompts"); it IS
 * HF's result for the row at batch size 1.
 *
 * n_pad_host == NULL or all zeros: the call IS tw_generate_greedy, launch for launch.  Otherwise the prompt is consumed one position per
 * step as there, a step issues one launch more (the embedding of a ragged step is a launch of its own; the embedding, the K / V cache
 * write and the self attention are instantiations of their own, every other launch is the plain step's), and captured step graphs are
 * kept apart from the plain call's.  Every context dtype is supported with the same equality, TW_BF16_MXFP8 (W8A8) included.  The table
 * lives in context-owned device memory, allocated by the first padded call of a context (a sibling owns its own) and freed by tw_destroy.
 *
 * TW_EINVAL in addition to tw_generate_greedy's, all before any work is enqueued (the context stays usable): a negative n_pad[b],
 * n_pad[b] >= n_prompt (a row needs one real token), n_forced or n_draft set in a padded call, B > 64.  tw_generate_greedy_biased,
 * tw_generate_sample* and tw_score_tokens take no padding. */
int tw_generate_greedy_ragged(tw_ctx* ctx, int32_t B, const int32_t* prompt_host, int32_t n_prompt, const tw_greedy_opts* opts,
                              const int32_t* n_pad_host /* [B] */, int32_t* out_ids_host, int32_t* out_len_host, void* stream);

/* Temperature sampling on the device.  Replaces: GenerationMixin._sample with do_sample=True and a TemperatureLogitsWarper behind
 * Whisper's logits processors (HF:generation/utils.py:1293-1312, :2925-2931), as WhisperGenerationMixin.generate_with_fallback invokes it
 * for the temperatures behind 0 (HF:models/whisper/generation_whisper.py:970-1116; thewhisper_amd/fallback.py restates that ladder).
 *
 * THE DRAW.  Row b consumes position p and produces the token at p + 1.  x = the float32 logits; the mask is exactly
 * tw_generate_greedy's, and "the timestamp mass beats every text token" is decided on the unscaled processed logits as there.  Among
 * the ids still unmasked
 *     score(v) = x[v] * inv_t[b] + g(v),    g(v) = -logf(-logf(u)),    u = ((w >> 9) * 2 + 1) * 2^-24   (exact, never 0 or 1),
 *     w = output word (v & 3) of Philox4x32-10, counter (v >> 2, p, offset low, offset high), key (seed low, seed high),
 * and the token is the lowest id that attains the maximum: Gumbel-max, a draw from softmax(x / T) over the unmasked ids.  Everything
 * masked: id 0, as the greedy call returns.  temperature[b]
 *     > 0 : sample, inv_t = 1.0f / T (computed on the host);
 *    == 0 : the row is greedy (no noise, inv_t = 1): its tokens are tw_generate_greedy's, bit for bit;
 *     < 0 : the row sits the call out: it starts finished, receives pad_id from position n_prompt on, never holds up the loop and
 *           does not count towards out_len_host.
 * The noise depends on (seed, offset, position, id) alone - not on the slot, the other rows of the batch or graph replay - so a
 * stream's result does not depend on what else is in its batch.  This is NOT torch's generator: no bit parity with
 * torch.multinomial is claimed or possible; and the draw is from the FULL distribution, as openai/whisper's, where HF's sampling
 * also applies top_k = 50 by default: tw_generate_sample_filtered below narrows the candidate set.
 *
 * Outputs as tw_generate_greedy's; want_alignment is honoured (tw_token_timestamps works after it); tw_last_timings[3] and the step
 * count are filled.  TW_EINVAL: n_forced or n_draft set, a NaN or infinite temperature or one so small that 1 / T is not finite, every
 * row < 0, a NULL temperature / seed, B outside 1 .. 64; TW_ESTATE, as tw_generate_greedy: B above the clips the cross K/V hold. */
typedef struct tw_sample_opts {
  const float*    temperature;  /* host float32 [B]; see "the draw" */
  const uint64_t* seed;         /* host [B]: Philox key */
  const uint64_t* offset;       /* host [B]: counter words 2, 3; NULL = all 0 */
} tw_sample_opts;
int tw_generate_sample(tw_ctx* ctx, int32_t B, const int32_t* prompt_host, int32_t n_prompt, const tw_greedy_opts* opts,
                       const tw_sample_opts* sopts, int32_t* out_ids_host, int32_t* out_len_host, void* stream);

/* tw_generate_sample with top-k and nucleus (top-p) filtering of the candidate set.  Replaces: the TopKLogitsWarper and
 * TopPLogitsWarper HF puts behind the TemperatureLogitsWarper, in that order (HF:generation/utils.py:1293-1321); top_k = 50 is what
 * HF's generate resolves to when nothing is set.
 *
 * THE RULE.  Row b at position p; x = the float32 logits after exactly the mask of tw_generate_sample, "the timestamp mass beats
 * every text token" included (decided on the unscaled logits, bit-equal to the greedy and unfiltered calls on equal logits); S = the
 * ids still unmasked.
 *   Top-k, top_k[b] = k > 0: tau = the k-th largest value of x over S, counted with multiplicity; tau = -inf if |S| <= k;
 *     K = { v in S : x[v] >= tau }.  Ties at tau are all kept (HF's `scores < topk(scores, k)[-1]` removes nothing equal to it).  The
 *     comparison is on the unscaled float32 x: scaling by inv_t > 0 is monotone, so only ties created by rounding could differ from
 *     HF, and x is what every other rule of this sampler is decided on.  K is an exact function of the logits.  k = 0: off (K = S);
 *     k > V acts as V.
 *   Top-p, 0 < top_p[b] < 1, applied to K: y[v] = x[v] * inv_t[b] rounded to float32 (the product the draw perturbs), m = max of y
 *     over K, e[v] = exp(y[v] - m), Z = sum of e over K, G(v) = sum of e[u] over the u in K with y[u] > y[v] (strict: equal values
 *     share their fate); v is kept iff G(v) < top_p * Z.  The maximum is always kept (HF's min_tokens_to_keep = 1).  In exact
 *     arithmetic this is HF's `cumsum(softmax(sorted ascending)) <= 1 - top_p` removal.  The library evaluates e in float32 and the
 *     sums in double precision; a membership whose G / Z lies within about 1e-5 of top_p may fall either way.  top_p = 1: off.
 *   The token is the lowest id that attains the maximum of score(v) = x[v] * inv_t[b] + g(v) over the kept ids: the noise is
 *     tw_generate_sample's, the same Philox words for (seed, offset, position, id).
 * Rows with temperature 0 are greedy and ignore the filters (the arg-max is always kept); rows with a negative temperature sit the
 * call out; everything masked: id 0.  A row with both filters off produces tw_generate_sample's token for the same seed, bit for bit,
 * whatever the other rows set.  fopts == NULL, or no sampled row with a filter on: the call IS tw_generate_sample, launch for launch.
 * Otherwise a step issues one launch more (the row is filtered in the registers of one workgroup) and captured step graphs are kept
 * apart from the unfiltered call's.  The filter holds vocabularies of up to 65536 ids (every Whisper vocabulary fits).
 *
 * Outputs, want_alignment, timings, the step count and the error codes as tw_generate_sample's.  TW_EINVAL in addition: a negative
 * top_k, a top_p that is NaN or outside (0, 1], a filter on in a context whose vocabulary exceeds 65536 ids. */
typedef struct tw_filter_opts {
  const int32_t* top_k;   /* host [B]; 0 = off; NULL = off for every row */
  const float*   top_p;   /* host [B]; 1.0f = off; NULL = off for every row */
} tw_filter_opts;
int tw_generate_sample_filtered(tw_ctx* ctx, int32_t B, const int32_t* prompt_host, int32_t n_prompt, const tw_greedy_opts* opts,
                                const tw_sample_opts* sopts, const tw_filter_opts* fopts, int32_t* out_ids_host,
                                int32_t* out_len_host, void* stream);

/* Beam search on the device with the n-best list.  Replaces: GenerationMixin._beam_search (HF:generation/utils.py:2976-3560) for
 * num_beams = K in 2 .. 8 with Whisper's logits processors, as WhisperGenerationMixin.generate_with_fallback invokes it for
 * generate_kwargs={"num_beams": K} (HF:models/whisper/generation_whisper.py:1027).
 *
 * THE RULE.  n_clips clips, K beams each, n0 = n_prompt, max_len = min(max_length, n0 + max_new_tokens, target_positions); all scores
 * float32.  Per clip: run_seq[K] = the prompt K times, run_score = [0, -1e9, ..], fin_seq[K] = the prompt then pad_id,
 * fin_score[K] = -1e9, fin_flag[K] = false, open = true, cur = n0.  One step consumes position cur - 1 of every beam:
 *   1. x_k = beam k's float32 logits; lp_k[v] = x_k[v] - m_k - log(sum_v exp(x_k[v] - m_k)) over all V ids, m_k = max x_k (HF's
 *      log_softmax, before any processor).
 *   2. The processors of `opts` on lp_k with history run_seq[k] and begin index n0: exactly tw_generate_greedy's mask, "timestamp mass
 *      beats every text token" included.  A masked id is -inf, every other id keeps its bits (no renormalisation).
 *   3. a[k V + v] = lp_k[v] + run_score[k] (one float32 add).  Candidates j = 0 .. 2K-1: the 2K largest a, descending, the lower flat
 *      index first on equal values (torch.topk leaves ties open): score s_j, source beam b_j, id t_j, sequence run_seq[b_j] + [t_j].
 *   4. hit_j = t_j == eos_id || cur + 1 >= max_len.
 *   5. r_j = hit_j ? s_j + (-1e9f) : s_j.  The K largest r_j (descending, lower j first) become run_seq / run_score; their b_j are
 *      beam_idx[K].
 *   6. f_j = s_j / pen[cur + 1 - n0], pen[g] = (float)pow((double)g, (double)length_penalty), one correctly rounded float32 division;
 *      then -1e9f is added once for each of: early_stopping and all of fin_flag; !open; !(j < K && hit_j).  The new finished set is the
 *      K largest of [fin_score[0 .. K-1], f_0 .. f_{2K-1}] (descending, lower index of that concatenation first); a chosen candidate's
 *      flag is j < K && hit_j.
 *   7. Every self-attention cache row of beam k becomes that of beam beam_idx[k]; cur += 1.
 *   8. open = open && any_k(run_score[0] / pen[cur - n0] > (fin_flag[k] ? min(fin_score) : -1e9f)).
 *   9. The clip is over - its state frozen - when !open, or early_stopping and all of fin_flag, or every hit_j held.
 * fin_seq[0] / fin_score[0] is the best hypothesis, fin_seq[0 .. K-1] the n-best list in descending score; an entry whose score is
 * <= -1e9 is a placeholder.  Deviation: where float32 rounding maps two different logits of one beam onto the same accumulated score,
 * the larger logit is listed first (the rule says the lower id); real ties between equal logits follow the rule.
 *
 * Rows: beam k of clip c is row (slot) k * n_clips + c.  The call copies every clip's cross K / V to the slots of its beams >= 1 and
 * never writes slots 0 .. n_clips-1: afterwards the context holds the n_clips clips as tw_cross_kv left them (tw_score_tokens and
 * further tw_generate_* calls for them need no re-encoding); whatever slots n_clips .. n_clips * K - 1 held is gone.  A step is the
 * ordinary decoder pass over n_clips * K rows plus four short launches (slice partials, one workgroup per clip for steps 3-6 / 8 / 9,
 * the in-place cache reorder, the position); steps are not captured, so use_graph contexts run the same launches.  A clip's result
 * does not depend on its slot or on its batch-mates.  tw_last_timings[3] and the step count are filled; the state tables live in
 * context-owned device memory, allocated by the first beam call of a context (a sibling owns its own) and freed by tw_destroy.
 *
 * out_ids_host [n_clips, max_length]: the best hypotheses.  out_len_host: int32 [2], ALWAYS two entries (unlike the other tw_generate_*
 * calls): [0] the common length of the best hypotheses (n0 + the longest generated part), [1] the common length of all K hypotheses
 * of all clips, written whether or not the n-best list is asked for.  out_score_host [n_clips] (may be NULL); out_nbest_ids_host
 * [n_clips, K, max_length] (may be NULL) and out_nbest_score_host [n_clips, K] (may be NULL).  Everything behind a hypothesis's end
 * is pad_id.
 * TW_ESTATE: tw_encode + tw_cross_kv did not fill n_clips slots.  TW_EINVAL, before any work is enqueued (the context stays usable):
 * num_beams outside 2 .. 8, n_clips * num_beams above max_batch or above 64, a NaN or infinite length_penalty, early_stopping outside
 * {0, 1}, want_alignment / n_forced / n_draft set, a TW_BF16_MXFP8 / TW_BF16_W8A16 context, a context whose target_positions exceed
 * 512 (the histories a workgroup holds), tw_generate_greedy's own refusals. */
typedef struct tw_beam_opts { int32_t num_beams; float length_penalty; int32_t early_stopping; } tw_beam_opts;   /* 2..8, finite, 0 | 1 */
int tw_generate_beam(tw_ctx* ctx, int32_t n_clips, const int32_t* prompt_host /*[n_clips, n_prompt]*/, int32_t n_prompt,
                     const tw_greedy_opts* opts, const tw_beam_opts* bopts,
                     int32_t* out_ids_host /*[n_clips, max_length] best*/, int32_t* out_len_host /*[2]*/, float* out_score_host /*[n_clips], may be NULL*/,
                     int32_t* out_nbest_ids_host /*[n_clips, K, max_length], may be NULL*/, float* out_nbest_score_host /*[n_clips, K], may be NULL*/,
                     void* stream);

/* tw_generate_beam with the alignment rows of every hypothesis, for token and word timestamps of a beam result.  Replaces:
 * WhisperGenerationMixin._extract_token_timestamps on a beam output (HF:models/whisper/generation_whisper.py:265-301: the
 * cross-attention rows of every beam at every step, gathered along beam_indices) - without a second pass through the decoder.
 *
 * opts->want_alignment == 0: the call IS tw_generate_beam, launch for launch, with the same bits (out_hyp_len_host is still filled).
 * want_alignment == 1: every step (the prompt steps too) records the alignment-head rows of every beam where the beam sits - row
 * (slot, position) of the buffer tw_get_alignment reads is written once and never moved while the loop runs - and the loop keeps the
 * ancestry: per step the source beam of every running beam (step 5's beam_idx), per finished entry the beam whose logits produced
 * its last token; the entry keeps it as it moves through the finished set (step 6).  Ids and scores are tw_generate_beam's, bit for
 * bit.  Before the call returns ONE more launch gathers the rows in place among the K slots of each clip.
 *
 * THE RULE.  Hypothesis h of `len` tokens (prompt included), n0 = n_prompt:
 *   - its alignment row at position p, 0 <= p <= len - 2, is the row that the beam which produced token h[p + 1] recorded at the
 *     step that consumed position p;
 *   - its DTW matrix (tw_token_timestamps_each) is rows n0 .. len - 2: N = len - 1 - n0 rows of its own, no row of any other
 *     hypothesis or clip; N <= 0 gives all zeros (HF :338-339); a placeholder (score <= -1e9, nothing generated) is such a row;
 *   - the result of a clip depends neither on its slot nor on its batch-mates.
 * That is: a hypothesis gets the timestamps HF gives it when its clip is decoded ALONE (the precedent is the ragged-prompt rule of
 * tw_generate_greedy_ragged).  Deviation from HF's BATCHED call: past a hypothesis's end HF replaces beam_indices == -1 by 0, i.e.
 * by global row 0 (beam 0 of clip 0), and those rows enter the hypothesis's z-score over the token axis and its DTW.  Checked on the
 * CPU with transformers 5.15.0 on the 139 (case, clip) pairs of tests/beam_judge.py: for all 76 clips whose best hypothesis is
 * shorter than the longest of its batch, HF's batched token timestamps differ from HF's timestamps for the same clip decoded alone;
 * on all 139, HF's batch-of-one timestamps equal the numpy oracle's (a teacher-forced decode of the best hypothesis, then its DTW)
 * to 1e-6.
 *
 * Afterwards slot k * n_clips + c holds rows 0 .. len - 2 of hypothesis k of clip c, so the best hypotheses sit in slots
 * 0 .. n_clips - 1; rows of a placeholder and rows at or behind len - 1 are unspecified.  tw_get_alignment and tw_score_tokens work
 * as after a greedy call with want_alignment (tw_score_tokens leaves the rows alone).  The ancestry tables live in context-owned
 * device memory beside the beam state (allocated by the first such call, freed by tw_destroy).  No atomics.
 * out_hyp_len_host [n_clips, K] (may be NULL): len of every hypothesis (n_prompt for a placeholder).
 * TW_EINVAL as tw_generate_beam, except that want_alignment == 1 is accepted - and refused when the context has no alignment heads. */
int tw_generate_beam_aligned(tw_ctx* ctx, int32_t n_clips, const int32_t* prompt_host /*[n_clips, n_prompt]*/, int32_t n_prompt,
                             const tw_greedy_opts* opts, const tw_beam_opts* bopts, int32_t* out_ids_host, int32_t* out_len_host /*[2]*/,
                             float* out_score_host, int32_t* out_nbest_ids_host, float* out_nbest_score_host,
                             int32_t* out_hyp_len_host /*[n_clips, K], may be NULL*/, void* stream);

/* Of the most recent tw_generate_greedy with n_draft > 0 (all streams together): draft tokens offered, draft tokens confirmed, rows-mode
 * launches and verify rounds it took.  Any pointer may be NULL.  No reference counterpart (see tw_greedy_opts::n_draft). */
int tw_last_draft(tw_ctx* ctx, int32_t* offered, int32_t* accepted, int32_t* launches, int32_t* rounds);

/* How the most recent call of the tw_generate_greedy / tw_generate_sample family consumed its prompt: the rows-mode launches it took
 * (0: one position per step) and the prompt positions those launches consumed.  The plain greedy call (no forced, draft, bias, repeat,
 * ragged or sampling options) with n_prompt >= 2 takes a prompt of at most 64 rows (n_prompt x n_clips; 16 in W8A8 contexts) as one
 * launch; the result is the step path's, bit for bit.  A call with n_forced > 0 reports its batched prefill (positions 0 .. n_prompt - 2);
 * the rows launches of a draft are tw_last_draft's.  Any pointer may be NULL. */
int tw_last_prompt_rows(tw_ctx* ctx, int32_t* launches, int32_t* positions);

/* Token log-probabilities and the no-speech probability of FINISHED sequences, by a teacher-forced re-scoring pass.  Replaces: the
 * `scores` HF's generate keeps per step and WhisperGenerationMixin._retrieve_avg_logprobs reduces
 * (HF:models/whisper/generation_whisper.py:1957-1974: log_softmax of the PROCESSED scores, gathered at the chosen tokens, summed and divided
 * by length + 1), and WhisperNoSpeechDetection (HF:generation/logits_process.py:2050-2112).  The greedy loop keeps no logits; this call runs
 * positions 0 .. seq_len-2 of ids_host through the decoder again in launches of up to 64 rows (streams x consecutive positions, 16 rows in
 * TW_BF16_MXFP8 contexts) whose logits are bit for bit the one-position step's, and reduces every row on the device.
 *   ids_host: int32 [B, ld], the first seq_len of every row are used (e.g. the out_ids of tw_generate_greedy, ld = max_length,
 *   seq_len = out_len); n_prompt = the begin index of the generation: n_prompt < seq_len <= target_positions, ld >= seq_len.
 *   out[b, p], n_prompt <= p < seq_len, is the natural-log probability of ids[b, p] given ids[b, :p]:
 *     out_logprob_raw_host  softmax of the logits as the model produced them;
 *     out_logprob_host      softmax of the logits after the processors `opts` describes, applied for the history ids[b, :p] exactly as
 *                           tw_generate_greedy applies them (suppress lists, begin-suppress at p = n_prompt, the min_new_tokens <eos>
 *                           mask, the timestamp pairing / monotonic / initial rules, "timestamp mass beats every text token");
 *                           -inf where ids[b, p] itself is masked.  This is the number HF averages into avg_logprob.
 *   Entries with p < n_prompt are 0.0f, and so are the entries behind a row's first opts->eos_id at p >= n_prompt (the padding; the <eos>
 *   itself is scored).  Both are float32 [B, seq_len] (row stride seq_len) and may be NULL.
 *   Of `opts` only eos_id, pad_id, min_new_tokens and the processor fields (timestamps, no_timestamps_id, max_initial_timestamp_index, the
 *   two suppress lists) are read; n_forced, n_draft, want_alignment and max_* are ignored.  opts = NULL: raw numbers only
 *   (out_logprob_host must be NULL) and no <eos> is known, so nothing counts as padding.
 *   no_speech_id >= 0: out_no_speech_host[b] (float32 [B], may be NULL) = softmax(raw logits of position no_speech_pos)[no_speech_id],
 *   0 <= no_speech_pos < seq_len - 1; no_speech_id < 0: off, out_no_speech_host is not written.
 * Deviation: HF reads the no-speech probability from a SECOND model call on the decoder inputs
 * (:2094-2110, logits[:, 0] when the prompt is longer than one token); here it is read from the teacher-forced pass at the position
 * the caller names - position 0 sees the same first token, and the decoder is causal, so it is the same distribution.
 * Requires tw_cross_kv for B slots (else TW_ESTATE).  Overwrites the self-attention caches, the decoder position and the logits;
 * leaves alone the alignment rows, tw_last_timings, tw_last_draft, the captured step graphs and everything the next
 * tw_generate_greedy depends on: tw_token_timestamps may be called before or after it.  Synchronises the stream once, at the end. */
int tw_score_tokens(tw_ctx* ctx, int32_t B, const int32_t* ids_host, int32_t ld, int32_t seq_len, int32_t n_prompt,
                    const tw_greedy_opts* opts, int32_t no_speech_id, int32_t no_speech_pos, float* out_logprob_host,
                    float* out_logprob_raw_host, float* out_no_speech_host, void* stream);

/* A11.  Replaces: _extract_token_timestamps + _median_filter + _dynamic_time_warping
 * (HF:models/whisper/generation_whisper.py:241-381, :43-61, :64-115) on the alignment rows recorded by the
 * last tw_generate_greedy(want_alignment=1).  num_frames_host[b] = valid mel frames: the time columns of row b are
 * cropped ONCE with Python-slice semantics `[: num_frames // 2]` (floor division; a negative bound counts from the end;
 * nothing left = HF's DTW on the empty matrix: every generated token at -1 * time_precision).  HF itself applies that
 * slice once or twice depending on the type and uniformity of its `num_frames` argument (:310-330, :357-359); which
 * bound reproduces HF's result for a given generate() batch is the host mirror's business
 * (thewhisper_amd/shortform.py::hf_kept_columns).  out_ts_host: float32 [B, seq_len] seconds (seq_len = out_len of the greedy call). */
int tw_token_timestamps(tw_ctx* ctx, int32_t B, int32_t n_prompt, int32_t seq_len, const int32_t* num_frames_host,
                        double time_precision, float* out_ts_host, void* stream);
/* tw_token_timestamps for rows of different lengths (the hypotheses of tw_generate_beam_aligned): seq_len_host[b] tokens in row b,
 * out_ts_host float32 [B, ld].  Row b is computed on its own N_b = seq_len[b] - 1 - n_prompt rows (positions n_prompt ..
 * seq_len[b] - 2 of slot b) and is, in its first seq_len[b] entries, bit for bit what tw_token_timestamps returns for that row alone
 * with seq_len = seq_len[b]: entries below n_prompt are 0, entries from seq_len[b] - 1 to ld - 1 repeat the row's last jump time,
 * N_b <= 0 gives zeros.  With every length equal to ld the call is tw_token_timestamps.  The three kernels take a nullable per-row
 * length; without it they run the code of the common-length call.
 * TW_EINVAL, before anything is enqueued: a seq_len[b] above ld or above target_positions (or negative), n_prompt < 1, ld < 1. */
int tw_token_timestamps_each(tw_ctx* ctx, int32_t B, int32_t n_prompt, const int32_t* seq_len_host /*[B]*/, int32_t ld,
                             const int32_t* num_frames_host, double time_precision, float* out_ts_host /*[B, ld]*/, void* stream);
/* Debug/parity access: copy the recorded alignment rows [B, n_align_heads, n_rows, T] (float32) to host. */
int tw_get_alignment(tw_ctx* ctx, int32_t B, int32_t n_rows, float* out_host, void* stream);
/* Its mirror: copy host float32 [B, n_align_heads, n_rows, T] into rows 0 .. n_rows-1 of slots 0 .. B-1 of the recorded-alignment
 * buffer (every other row keeps what it held), so that tw_token_timestamps can be run on a chosen surface without a decode.
 * Same argument checks and error codes as the getter; synchronises the stream once. */
int tw_set_alignment(tw_ctx* ctx, int32_t B, int32_t n_rows, const float* in_host, void* stream);

/* Per-stage device timings (milliseconds, HIP events on the call's stream) of the most recent call
 * of each kind: [0]=logmel [1]=encode [2]=cross_kv [3]=greedy loop [4]=token_timestamps; also the
 * number of decode steps of the last greedy call in steps_out.  Used by bench.py for the roofline. */
int tw_last_timings(tw_ctx* ctx, float* ms_out5, int32_t* steps_out);

/* SURVEY 8f-2.  Stands where the reference calls silero-vad: `prob = vad_model(frame_512, 16000).item()` on consecutive
 * 512-sample frames with state kept between calls (R:thestage_speechkit/streaming/streaming_pipeline.py:533-538, :589-622).
 * NOT silero (its weights are not obtainable offline): an adaptive-noise-floor energy detector with the same contract, rule in
 * thewhisper_amd/csrc/k_vad.hip.  pcm_dev: float32 [B, stream_stride] (16-byte aligned), the first n_frames*512 samples of
 * every row are processed in order; state_dev: float32 [B, 2] (noise floor dB, started flag; zero-initialise to reset a
 * stream); prob_dev: float32 [B, n_frames].  Asynchronous on `stream`. */
int tw_vad_energy(int32_t device, const float* pcm_dev, int64_t stream_stride, int32_t B, int32_t n_frames, float* state_dev,
                  float* prob_dev, void* stream);

/* Front end.  Stands where the reference resamples a client's audio to 16 kHz with librosa before its pipeline sees it
 * (R:thestage_speechkit/streaming/streams.py:103-105, R:examples/run_nvidia_asr.py:30).  NOT a port of librosa / soxr: a rational
 * polyphase Kaiser-windowed-sinc resampler of this project's own definition (thewhisper_amd/csrc/k_resample.hip), context-free
 * like tw_vad_energy.  Supported: sr_in, sr_out >= 4000 whose prototype table (2 * 16 * max(L, M) + 1 taps, L / M = sr_out / sr_in
 * in lowest terms) is at most 1 MiB of float32; sr_in == sr_out is a bit-exact copy (after conversion and down-mix). */
enum { TW_PCM_F32 = 0, TW_PCM_S16 = 1 };   /* S16: little-endian int16, value / 32767 */
/* Host only, no GPU needed: L, M, half (prototype half-width in taps) and taps per output of the (sr_in -> sr_out) plan - what a
 * caller of R:thestage_speechkit/streaming/streams.py:103-105 never sees of librosa's filter.  Any pointer may be NULL. */
int tw_resample_plan(int32_t sr_in, int32_t sr_out, int32_t* L, int32_t* M, int32_t* half, int32_t* taps_per_output);
/* Host only: the n = 2*half+1 prototype taps in double, exactly what the device table is rounded from (the filter that replaces
 * librosa's inside R:thestage_speechkit/streaming/streams.py:103-105). */
int tw_resample_taps(int32_t sr_in, int32_t sr_out, double* out_host, int32_t n);
/* Replaces: `librosa.resample(chunk, orig_sr=sr, target_sr=16000)` (R:thestage_speechkit/streaming/streams.py:103-105) and the
 * int16 / channel handling in front of it, for B rows in ONE launch.  in_dev: [B, in_stride_frames, channels] of in_fmt,
 * interleaved; the channels of a frame are averaged in float32 before filtering.  Row b holds in_count_host[b] frames, the first
 * of which is frame in_first_host[b] of its stream; frames outside that window or before frame 0 read as zero.  out_dev:
 * float32 [B, out_stride]; row b receives output samples out_first_host[b] .. out_first_host[b] + n_out - 1 of its stream
 * (y[n] = sum_k x[k] h[n M - k L]).  A pure function of its arguments: streaming state (a tail of input, two counters) is the
 * caller's (thewhisper_amd/resample.py), and a sample's bits do not depend on B or on how the stream was cut.  1 <= B <= 64,
 * 1 <= channels <= 8.  Asynchronous on `stream`. */
int tw_resample(int32_t device, const void* in_dev, int32_t in_fmt, int32_t channels, int64_t in_stride_frames,
                const int64_t* in_first_host, const int32_t* in_count_host, int32_t sr_in, int32_t sr_out,
                const int64_t* out_first_host, int32_t n_out, float* out_dev, int64_t out_stride, int32_t B, void* stream);

/* Host-side schedule helpers (no reference counterpart: the reference processes one request at a time,
 * R:examples/server.py:22-115).  Streams and events created by the SAME HIP runtime the library and torch use, for the
 * encoder / decoder stage overlap (thewhisper_amd/overlap.py): a stream whose kernels may only run on the compute units
 * set in `cu_mask` (n_words x 32 bits), plain events, record / wait.  Handles are hipStream_t / hipEvent_t as void*. */
int tw_stream_create_masked(int32_t device, const uint32_t* cu_mask, int32_t n_words, void** out_stream);
int tw_stream_destroy(void* stream);
int tw_stream_synchronize(void* stream);
int tw_event_create(int32_t device, void** out_event);
int tw_event_destroy(void* event);
int tw_event_record(void* event, void* stream);
int tw_stream_wait_event(void* stream, void* event);

#ifdef __cplusplus
}
#endif
#endif /* THEWHISPER_H */
