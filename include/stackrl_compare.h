/* stackrl_compare.h — C-ABI of libstackrl_compare.so: the statistics that compare the value maps of several policies.
 *
 * The reference's `test` command (stackrl/test.py) lets each of P policies drive the env in turn while every policy evaluates
 * every observation, keeps all value maps as a float32 array [P][P * num_steps][A] (:221-224) and reduces it afterwards
 * (`analyse`, :412-721) to a few P x P matrices: the correlation of the value functions (:603) and the overlap of the actions
 * valued above a map's mean and above its mean + std (:616-656).  Here every vectorised step is reduced where its maps lie, in
 * one pass per env, to a fixed record of sums and counts; the matrices are computed from the record at the end.
 *
 * THE DEFINITION (stated here once; `stackrl_amd.compare.compare_reference` restates it in numpy float64, `MapStatistics`
 * computes it in torch on the CPU and with the kernel `k_compare` of csrc/compare.hip on the device):
 *
 *   One step holds P policies (1..8), B envs and A actions.  Policy j's maps are [B][G][A] (G object maps per env: the
 *   orientations of Stack-v2, the map of the chosen row is used, row = actions[j][b] / A clamped to 0..G-1; G = 1 and no
 *   actions otherwise), float32 or float64 elements per policy.
 *     x[j][b][a]  = the element rounded to float32 (test.py:277-280 assigns into a float32 array)
 *   per (j, b):
 *     amax[j][b]  = the maximum of x[j][b][:] in float32; NaN if the map holds a NaN (numpy's max, :455)
 *     mu          = (sum_a x) / A                        the sum accumulated in float64
 *     sigma       = sqrt((sum_a (x - mu)^2) / A)         float64, the population standard deviation (ddof 0)
 *     f1[a]       = x > mu          f2[a] = x > mu + sigma         (float64 comparisons; a NaN on either side: false)
 *   per env and per pair i <= j, in the order (0,0), (0,1), ..., (0,P-1), (1,1), ..., (P-1,P-1):
 *     S[i][j]     = sum_a x_i * x_j                      float64 (each product of two float32 values is exact)
 *     I1, U1      = the number of actions with f1_i and f1_j / f1_i or f1_j;   I2, U2: the same with f2
 *     s[j]        = sum_a x_j
 *   The record, float64[R(P)] with NP = P (P + 1) / 2 and R(P) = 1 + P + 5 NP, sums these over envs and steps:
 *     [0] envs seen (steps * B)   [1 ..] s[P]   then S[NP], I1[NP], U1[NP], I2[NP], U2[NP]
 *   Every sum has a fixed order: a thread's elements in ascending index, a shuffle tree inside each wave, the four waves
 *   in wave order, then the envs of a step in env order onto the running record.  No float atomics: the same inputs give
 *   the same record bit for bit.  Counts are exact integers in float64 (up to 2^53).
 *
 *   From a record, with n = record[0] * A and m = s / n:
 *     cov      = S / n - m m^T,   d = diag(cov),   corrcoef = cov / sqrt(d d^T), clipped to [-1, 1] (np.corrcoef, :603)
 *     overlap  = I / U                                                            (:619-656)
 *   NaN and +-inf take the way IEEE arithmetic gives them, as in the numpy lines: a map with a NaN has a NaN threshold and
 *   no flagged action; a constant map has d = 0 (if its sums are exact) and its correlations are NaN, np.corrcoef's 0 / 0,
 *   also where the rounding of S / n and m m^T left a non-zero numerator over that zero.
 *
 * Plain C, device pointers owned by the caller, contiguous, `stream` is a hipStream_t as void*; returns 0 on success.
 */
#ifndef STACKRL_COMPARE_H_
#define STACKRL_COMPARE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRL_COMPARE_MAX_POLICIES 8

/* R(P), the number of float64 of a record; 0 for P outside 1..8. */
int32_t srl_compare_record_doubles(int32_t P);

/* One step.  map0..map7: the maps of policy 0..P-1 (the others are not read), [B][G][A], float64 where bit j of f64_mask is
 * set and float32 otherwise; actions int64 [P][B] or NULL (row 0 of every env); amax float32 [P][B] (out); partial float64
 * [B][R(P)] (scratch, overwritten); record float64 [R(P)] (read and written: the step is added to it; zero it before the
 * first step).  P outside 1..8, B, G or A below 1, G * A beyond 2^31 - 2, a null map among the first P, a null amax, partial
 * or record return 1 and launch nothing; a launch error returns 4.  The message is read through srl_compare_last_error. */
int srl_compare_step(int32_t P, const void* map0, const void* map1, const void* map2, const void* map3, const void* map4,
                     const void* map5, const void* map6, const void* map7, int32_t f64_mask, int32_t B, int32_t G, int32_t A,
                     const int64_t* actions_dev, float* amax_dev, double* partial_dev, double* record_dev, void* stream);

const char* srl_compare_last_error(void);
const char* srl_compare_build_info(void);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_COMPARE_H_ */
