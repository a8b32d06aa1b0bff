/* stackrl_explore.h — C-ABI of libstackrl_qnet.so, continued: the Boltzmann exploration head of the rollout path.
 *
 * The reference's Boltzmann branch of `DQN.policy` (stackrl/agents/dqn.py:349-358) is the Gumbel-max trick:
 * `argmax_a(Q(s,a) / T - log(-log(uniform)))` samples `a` with probability softmax(Q / T).  Here the uniform numbers
 * belong to the SAMPLE, not to the call: a batch evaluated in any partition (chunks, env groups, a permutation) takes the
 * actions of one call over the whole batch, and no [B][A] noise tensor exists.
 *
 * THE NOISE DEFINITION (stated here once; `stackrl_amd.dqn.philox4x32_10` / `boltzmann_noise` restate it in torch for
 * either device, the kernel `k_boltzmann_head` of csrc/qnet.hip computes it):
 *
 *   sample b owns a 64-bit stream key (k0, k1), two 32-bit words; for its action a
 *     x     = Philox4x32-10(counter = (a / 4, 0, 0, 0), key = (k0, k1))[a % 4]
 *             (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85 between the ten rounds)
 *     u     = ((x >> 9) + 0.5) * 2^-23       every value exact in float32 and within [2^-24, 1 - 2^-24]: neither
 *                                            logarithm sees 0 or 1.  (24 bits would not do: ((x >> 8) + 0.5) * 2^-24
 *                                            needs 25 mantissa bits and rounds to 1.0 at the top.)
 *     z     = -log(-log(u))
 *     score = adv[a] / T + z                 in float32
 *   action  = argmax_a score, ties to the lowest index.
 *
 * `adv` is the advantage map: the dueling mean and the value are constant per row (models.py:188-192) and do not change
 * the arg-max, as for srl_policy_head.  T is the temperature (`DQN.exploration`) rounded to float32.
 *
 * Plain C, device pointers owned by the caller, `stream` is a hipStream_t as void*; returns 0 on success.
 */
#ifndef STACKRL_EXPLORE_H_
#define STACKRL_EXPLORE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* adv float32 [B][A], keys int64 [B][2] (the low 32 bits of each element are the key word), actions int64 [B]; contiguous.
 * A null pointer, B < 1, A < 1 or a temperature that is not > 0 (NaN included) return 1 and launch nothing; a launch error
 * returns 4.  The message is read through srl_qnet_last_error (stackrl_qnet.h). */
int srl_boltzmann_head(const float* adv_dev, const int64_t* keys_dev, float temperature, int64_t* actions_dev, int32_t B,
                       int32_t A, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_EXPLORE_H_ */
