/* stackrl_baseline_rows.h — C-ABI of libstackrl_qnet.so, continued: the heuristic baselines on Stack-v2, where one env's
 * observation holds G object maps (the orientations of the pending rock, or rock x orientation under ordering freedom)
 * over ONE overhead map, and the policy chooses (object map, pixel).
 *
 * The reference's `test` command builds `Baseline(method, value=True, batched=True, batchwise=True)` for such observations
 * (stackrl/__main__.py:90-117): `PyGreedy.__call__` (stackrl/agents/policies.py:57-91) runs `Baseline.call`
 * (stackrl/baselines.py:201-217) on every object map and keeps the map whose returned (negated) value at its own action is
 * the largest.  That is not an arg-min over all maps' raw values: the goal-overlap mask and the local-minimum rule act per map.
 *
 * THE DEFINITION (stated here once; `stackrl_amd.baselines.baseline_rows_reference` restates the selection in numpy float64 on
 * the CPU, the kernels `k_heuristic_rows` and `k_baseline_rows_select` of csrc/heuristics.hip compute it):
 *
 *   env b holds G rows of which the first n_valid are valid; A = (H - h + 1)^2.  For a valid row r
 *     values[b][r][.], mask[b][r][.]  = what srl_heuristic (stackrl_qnet.h) returns for the observation
 *                                       (obs_map[b], obs_obj[b][r]): the same float64 operations in the same order, so the
 *                                       same bits.  The goal maximum gmax, the table k / gmax and the flags height < goal
 *                                       are taken from obs_map[b]: they belong to the env, not to the row.
 *     a_r                             = the action srl_baseline_select returns for that row (use_goal, minorder)
 *     neg[b][r][.]                    = the map srl_baseline_select returns for that row
 *     c[b][r]                         = neg[b][r][a_r]
 *   r*         = the lowest r that maximises c[b][r]                          (np.argmax(max_list), policies.py:79)
 *   actions[b] = r* * A + a_{r*}
 *   Rows r >= n_valid are never read (with ordering freedom the reference's observation has no such rows, env.py:596-608);
 *   their values and mask are not written, their neg and their c are -inf.
 *   An env whose goal channel is all zero has gmax = 0 as in srl_heuristic: NaN values and an arbitrary action in that env;
 *   the other envs of the batch are not touched by it.
 *
 * One workgroup computes one (env, row) value map; one workgroup per env scans its rows in order for the choice.  No
 * floating-point atomics; every reduction runs in a fixed order, so a result does not depend on how a batch is partitioned.
 *
 * Plain C, device pointers owned by the caller, contiguous, `stream` is a hipStream_t as void*.  Nothing is allocated and
 * nothing is synchronised.  Returns 0 on success, 1 for refused arguments (nothing is launched), 4 for a runtime or launch
 * error; the message is read through srl_qnet_last_error (stackrl_qnet.h).
 */
#ifndef STACKRL_BASELINE_ROWS_H_
#define STACKRL_BASELINE_ROWS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* method and the last four parameters as for srl_heuristic.  obs_map uint8 [B][H][H][2]; obs_obj uint8 [B][G][h][h];
 * values float64 [B][G][A]; mask uint8 [B][G][A] or NULL.  The grid covers (env, row < n_valid) only.  Refused: a null
 * obs_map, obs_obj or values, B outside 1..65535, G < 1, n_valid outside 1..G, h < 1, H < h, a method outside 1..4, and a map
 * whose staging does not fit one workgroup's LDS (H = 256 with h = 64). */
int srl_heuristic_rows(int32_t method, const uint8_t* obs_map_dev, const uint8_t* obs_obj_dev, double* values_dev,
                       uint8_t* mask_dev, int32_t B, int32_t G, int32_t n_valid, int32_t H, int32_t h,
                       int32_t difference_exponent, int32_t weights_exponent, int32_t localized, double threshold,
                       void* stream);

/* values float64 [B][G][OH * OH]; mask uint8 of the same shape (may be NULL if use_goal == 0); actions int64 [B];
 * chosen float64 [B][G] (c of the definition) or NULL; neg_values float64 [B][G][OH * OH] or NULL.  Refused: a null values
 * or actions, a null mask with use_goal, B < 1, G < 1, n_valid outside 1..G, OH outside 1..32768, minorder < 0. */
int srl_baseline_rows_select(const double* values_dev, const uint8_t* mask_dev, int32_t use_goal, int32_t minorder,
                             int32_t B, int32_t G, int32_t n_valid, int32_t OH, int64_t* actions_dev, double* chosen_dev,
                             double* neg_values_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_BASELINE_ROWS_H_ */
