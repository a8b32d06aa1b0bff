/* stackrl_greedy.h — C-ABI of libstackrl_qnet.so, continued: the greedy head of the rollout path (acting without
 * exploration, evaluation, the Stack-v2 choice among orientations).
 *
 * The reference's greedy policies (stackrl/agents/policies.py:4-37, `DQN.policy(values=True)` in `Training.eval`,
 * stackrl/train/training.py:398-452) take the arg-max of the whole Q tensor and, in evaluation, keep every step's [B][A]
 * values to print five numbers.  Here the head turns the advantage maps and the state value into the action and the
 * statistics of Q in one pass per env; the Q tensor is written only when asked for.
 *
 * THE DEFINITION (stated here once; `stackrl_amd.dqn.greedy_head_reference` restates it in torch for either device, the
 * kernel `k_greedy_head` of csrc/greedy.hip computes it):
 *
 *   env b holds G rows (object maps: the orientations of Stack-v2; G = 1 otherwise) of A advantages, of which the first
 *   n_valid are valid.  For a valid row r
 *     m_r        = float32( (sum_p adv[b][r][p], accumulated in float64) / A )
 *     q[b][r][p] = (adv[b][r][p] - m_r) + v[b]        both operations in float32, in this order (models.py:188-192:
 *                                                     `outputs - mean + v`)
 *   With v == NULL (a network without the dueling head) q = adv and no mean is taken.
 *   The float64 accumulation makes m_r independent of the summation order up to float64 rounding; one workgroup owns one
 *   env and reduces in a fixed order, so the result does not depend on how a batch is partitioned.
 *
 *   action[b] = arg-max of q over r < n_valid and all p, as the flat index r * A + p; ties go to the lowest flat index.
 *               A NaN never wins a comparison; if nothing wins (nothing but NaN or -inf) the action is 0 — the rule of
 *               srl_policy_head.
 *   stats[b]  = {max q, min q, sum q, sum q^2} over the valid rows, float64: max and min skip NaN (-inf / +inf if there
 *               is nothing else), the sums run over every valid element and are accumulated in float64.
 *   Rows r >= n_valid are never read (with ordering freedom the reference's observation has no such rows, env.py:596-608);
 *   if q is written, those rows are written as -inf, as `policies.OrientationGreedy` does.
 *
 * Plain C, device pointers owned by the caller, contiguous, `stream` is a hipStream_t as void*; returns 0 on success.
 */
#ifndef STACKRL_GREEDY_H_
#define STACKRL_GREEDY_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* adv float32 [B][G][A]; v float32 [B] or NULL; actions int64 [B]; stats float64 [B][4] or NULL; q float32 [B][G][A] or
 * NULL.  A null adv or actions, B, G or A below 1, n_valid outside 1..G or G * A beyond 2^31 - 2 return 1 and launch nothing;
 * a launch error returns 4.  The message is read through srl_qnet_last_error (stackrl_qnet.h). */
int srl_greedy_head(const float* adv_dev, const float* v_dev, int32_t B, int32_t G, int32_t n_valid, int32_t A,
                    int64_t* actions_dev, double* stats_dev, float* q_dev, void* stream);

/* The cross-correlation forward of the greedy path (`layers.correlation`, layers.py:21-38; 128 x 128 maps, 32 x 32 kernels, at
 * most 16 channels): in [B][C][128][128], kern [B][C][32][32], both bfloat16 (f32 = 0) or both float32 (f32 = 1), out float32
 * [B][97][97]; precision as for srl_xcorr_mfma (0 = operands rounded to bf16, 1 = the hi / lo split, float32 operands only).
 * srl_xcorr_mfma (stackrl_qnet.h) picks its kernel and the split of the channel sum over workgroups by the batch size, so a
 * sample's map depends — in the order of its float32 sums — on the batch it arrives in.  This entry point always launches the
 * row-product kernel (csrc/xcorr_mfma.hip k_xcorr_rows4, what srl_xcorr_mfma launches from 192 samples on): one workgroup per
 * sample, the same sums in the same order at every batch size.  Below 192 samples it leaves compute units idle; greedy acting
 * pays that for results that do not depend on how a batch is partitioned.  Bad arguments return 1 and launch nothing, a launch
 * error returns 2; the message is read through srl_xcorr_mfma_last_error (stackrl_qnet.h). */
int srl_xcorr_rows(int32_t precision, const void* in_dev, const void* kern_dev, int32_t f32, float* out_dev, int32_t B, int32_t C,
                   int32_t H, int32_t kh, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_GREEDY_H_ */
