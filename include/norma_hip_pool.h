/* norma_hip_pool.h -- the decode pool's extensions to the C ABI of norma_hip.h, same library (libnorma_hip.so), same
 * conventions: status codes, nh_last_error, one host thread per context.
 * Why a header of its own: the prototype list of norma_hip.h is pinned, name by name and by count, by tests/test_cabi_cpu.py and
 * (through INTEGRATION.md's first binding block) by tests/test_abi.py, and a change that adds a capability leaves existing
 * test files as they are.  So what the ABI gains is declared here, with its own binding block in INTEGRATION.md and its own
 * checks (tests/test_pool_prompt_cpu.py: the prototype, the bound types, export by both builds of the library); an embedder
 * that wants the pool's prefixes includes this header INSTEAD of norma_hip.h, which it pulls in.
 *   nh_pool_prefix                (no counterpart: every reference decode starts from [sot, lang?, task], model.rs:285-289)
 *                                 a prompt prefix per row of a decode pool, every row its own length, prefilled in one ragged pass
 */
#ifndef NORMA_HIP_POOL_H
#define NORMA_HIP_POOL_H

#include "norma_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The prefix of the clip that the NEXT nh_pool_admit / nh_pool_admit_from puts into `row`: n_prefix ids, taken verbatim, in
 * front of [sot, lang?, task] (conditioning on previous text: the caller puts <|startofprev|> first).  One-shot: that
 * admission consumes it; nh_pool_begin clears every pending one; tokens == NULL or n_prefix == 0 clears the row's.  Returns
 * when the caller's buffer is no longer needed; nothing is launched.
 * Per row it means what nh_set_prompts means for a batch: positions 0 .. n-1 consume the prefix, [sot, lang?, task] sit at
 * n .., the no-speech probe reads the logits at position n, generation starts at n + P - 1; the rules, the forced first
 * timestamp, max_new_tokens and the guard's history count from n + P; the length cap applies to the physical sequence; the
 * sampling counter `step` is the physical token count.  Tokens, avg_logprob and no_speech_prob of the row are bit for bit
 * those of nh_set_prompts + nh_decode_greedy on a lockstep batch that holds the clip with that prefix.  nh_pool_collect
 * returns the sequence from sot on: out_tokens and n_tokens exclude the prefix, avg_logprob is divided by that n_tokens.
 * nh_pool_retry restarts the row at position n on the self K/V that positions 0 .. n-1 left in its cache (nothing is computed
 * again): the bits of nh_decode_sampled under nh_set_prompts with the same prefix.
 * The route is chosen at the admission.  n >= 4 on a model the one pass covers and NH_OPT_PROMPT_STEPWISE == 0: the row starts
 * at position n, and the next nh_pool_step that runs steps first consumes the prefixes of all rows admitted since the last
 * one in ONE ragged one-pass forward.  Otherwise the row starts at position 0 and the pool's own steps consume the prefix
 * (nothing is selected at those positions); the lockstep yardstick is then the decode under NH_OPT_PROMPT_STEPWISE = 1.  A pool in
 * which no row has a prefix launches what it launched before.
 * Refused, nothing launched, pending prefixes and rows untouched: no pool (NH_ERR_STATE); row outside the pool or busy,
 * n_prefix outside 0 .. max_target_positions / 2 - 1, a token id outside the vocabulary (NH_ERR_INVALID).  nh_pool_admit*
 * with lang == NH_LANG_DETECT into a row with a pending prefix is NH_ERR_INVALID (the probe step behind a prefix is not
 * nh_detect_language's forward on [sot]); it and an admission refused for any other reason leave the prefix pending.
 * nh_align_decoded on a row whose last decode had a prefix is NH_ERR_STATE, as after a prompted lockstep decode. */
int nh_pool_prefix(nh_ctx *ctx, int row, const int32_t *tokens, int n_prefix);

#ifdef __cplusplus
}
#endif
#endif
