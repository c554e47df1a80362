// Every environment knob of libcapdec_hip.so in ONE place.  capdec_create parses the environment once into the context's
// Tuning (capi_context.hip: tuning_from_env); the launchers of the other translation units receive a pointer to it through
// GemmEpilogue::tune / their arguments -- no translation unit reads the environment on its own, nothing
// is latched in function-local statics, and two contexts created under different environments behave differently, as
// the tests that monkeypatch the environment expect.
//
// Every knob selects among correct code paths (A/B switches kept for regression hunting; every default is the
// measured-fastest setting, none is needed for normal use).  There are no measurement knobs: the ablations, ring-depth /
// occupancy overrides, extra tile geometries and phase stamps of rounds 2-6 gave their figures (profiles/, docs/rounds.md)
// and are gone together with every kernel variant only they reached.  The measurement library
// (capdec_amd/lib/libcapdec_hip_measure.so, used by bench.py's untimed tail and one parity test) is this library plus ONE
// exported function, capdec_set_debug_diverge (capi_context.hip, compiled a second time for it); it reads the same environment.
// Changed with that clean-up: CAPDEC_PP is a flag like its neighbours.  Its former modes 1 and 3 (also / only the 256 x 256
// tile for large launches, which only ever acted in measurement builds) are read as "on", the default; in the shipped
// library CAPDEC_PP=3 used to mean "never" for every reachable launch.
#pragma once
#include <string>

namespace capdec {

struct Tuning {
    int gemm_mode = 3;            // CAPDEC_GEMM_MODE: f32 0 | bf16x3 1 | bf16 2 | f16x2 3 (default) | f16 4
    bool batch_invariant = false; // CAPDEC_BATCH_INVARIANT
    bool compact = true;          // CAPDEC_COMPACT=0: finished captions stay in the batch
    bool x3_pack_a = true;        // CAPDEC_X3_PACKA=0: bf16x3 mode, LayerNorm writes fp32 (the GEMM splits A itself)
    bool pack_chain = true;       // CAPDEC_X3_CHAIN=0: attention / fc epilogue write fp32 instead of packed operands
    bool splitk = true;           // CAPDEC_SPLITK=0: no split-K at all
    bool splitk_mid = true;       // CAPDEC_SPLITK_MID=0: no split-K for mid-size batches
    bool x1_splitk = true;        // CAPDEC_X1_SPLITK=0: none for the one-plane (bf16 / f16) kernels
    bool fuse_ln = true;          // CAPDEC_FUSE_LN=0: separate split-K reduce and LayerNorm
    int h2_persist = 512;         // CAPDEC_H2_PERSIST: blocks of the persistent form (0 = one block per tile)
    int h2w = 1;                  // CAPDEC_H2W: 0 = round-2 kernels only, 1 = planners, 2 / 8 = force a round-3 wide tile,
                                  //             10 / 14 = force a round-4 ping-pong tile (tests)
    bool pp = true;               // CAPDEC_PP=0: no ping-pong tiles from the planner (default: mid-size launches take them)
    bool lmhead_wide = true;      // CAPDEC_LMHEAD_WIDE=0: 128-row lm_head tiles at every size
    bool lmhead_k3 = true;        // CAPDEC_LMHEAD_K3=0: the wide lm_head keeps k candidates per tile (no exact second pass)
    int lmhead_k3_max = 60;       // CAPDEC_LMHEAD_K3_MAX: per mille of the rows taking the second pass above which a decode
                                  //   call goes back to k per tile (checked at the poll points; break-even is ~80)
    int lmhead_sparse = 1;        // CAPDEC_LMHEAD_SPARSE: 0 = the 3-per-tile route where the default (1) keeps no candidates per tile at all
                                  //   and recomputes, per row, the five tiles that can hold its top 5 (k = 5, wide tile, >= 40 column
                                  //   tiles, from 12288 rows: LM_SPARSE_MIN_ROWS); 2 = that route from the wide tile's first row (tests)
    int sample_rows = 2048;      // CAPDEC_SAMPLE_ROWS: rows of fp32 logits the sampling decode (and a decode with logits processors) materialises at a time (2048 rows of
                                  //   GPT-2's vocabulary = 412 MB); a step with more rows loops lm_head + sampler over row blocks
    int score_rows = 16384;       // CAPDEC_SCORE_ROWS: padded activation rows (captions x (prefix + longest caption - 1)) one chunk of
                                  //   capdec_score pushes through the GPT-2 body at a time (16384 rows = 1.2 GB of K / V + 0.4 GB of
                                  //   activations at GPT-2 small); a chunk always holds at least one caption
    bool kv_direct = true;        // CAPDEC_KV_DIRECT=0: the attention kernel appends K / V itself
    bool clip_trunc = true;       // CAPDEC_CLIP_TRUNC=0: the CLIP text tower computes all 77 positions of every caption (default: only
                                  //   the positions up to a chunk's last EOT; captions sorted by length)
    bool rn_packed = true;        // CAPDEC_RN_PACKED=0: fp32 im2col in the ResNet tower
    bool rn_implicit = true;      // CAPDEC_RN_IMPLICIT=0: fp32 activations in the ResNet tower
    bool train_f16x2 = true;      // CAPDEC_TRAIN_F16X2=0: the train step's backward GEMMs on the native fp32 MFMA GEMM instead of the
                                  //   two-fp16-plane kernels (A/B: 39.4 vs 23.6 ms per step; both parity-tested)
    bool train_attn_blk = true;   // CAPDEC_TRAIN_ATTN_BLK=0: the train step's attention on the per-query wavefront kernels at every sequence
                                  //   length (the fallback above 128 positions) instead of the block-per-(sample, head) kernels
    bool hook_packa = false;      // CAPDEC_HOOK_PACKA: capdec_gemm_f32 (test hook) packs A first (the LayerNorm -> GEMM path)
    bool hook_cache = false;      // CAPDEC_HOOK_CACHE: ... and treats both operands as resident (micro-benchmarks)
    std::string rccl_lib;         // CAPDEC_RCCL_LIB: path of librccl for the C-ABI communicator
};

// parses the environment; on a malformed value returns false and sets *err (capdec_create then fails: a typo must not
// silently select another precision)
bool tuning_from_env(Tuning *t, std::string *err);
// what launchers use when their caller passes no Tuning (default-constructed: every default above)
const Tuning &default_tuning();

}  // namespace capdec
