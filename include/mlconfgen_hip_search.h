/* Pose search ("Pose search"): S keyed starts per posed molecule for the flexible walk of
 * mlconfgen_hip_flex.h, and the exact choice among the walked starts.  A fourth public header of libmlconfgen_hip.so: plain
 * C99 / C++, the conventions, error codes and stream contract of mlconfgen_hip.h, which it includes - with
 * mlconfgen_hip_flex.h - for the shared limits (MCG_RECEPTOR_MAX_B, MCG_FLEX_MAX_ATOMS, MCG_FLEX_MAX_TORSIONS,
 * MCG_FLEX_STATS).  Every entry returns 0 on success and MCG_ERR_ARG (1) with mcg_last_error() text for an argument it
 * refuses, before any launch.  `stream` is the hipStream_t the work goes to; nothing here synchronises, allocates or keeps
 * state.  The walk between the two entries is mcg_receptor_optimise_flex itself, on the B * S start rows.
 * The package's OWN procedure: a bounded multi-start of its own downhill walk - not a docking run, not AutoDock Vina's Monte
 * Carlo search. */
#ifndef MLCONFGEN_HIP_SEARCH_H
#define MLCONFGEN_HIP_SEARCH_H

#include "mlconfgen_hip.h"
#include "mlconfgen_hip_flex.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCG_SEARCH_MAX_STARTS 64  /* starts per molecule */
#define MCG_SEARCH_PARAMS 24      /* columns of start_params: the uniforms of draws j = 0..5, four each */

/* ---- S starts per molecule, one 64-lane wave per (molecule b, start s), lane = atom.
 *   lig_xyz[B,N,3], n_nodes_dev[B] (clamped to 0..N); torsion_atoms[B,16,2], side_mask[B,16]: mcg_torsion_tree's outputs for
 *   the same rows; n_torsions[B] the torsions to use, clamped to 0..16 and cut at the first slot whose atoms are not inside
 *   the row, as mcg_receptor_optimise_flex does.  sample_ids_dev[B] int64 in [0, 2^32); seed: the key; spread (A, >= 0) and
 *   max_turn (rad, 0..pi): the largest shift of the centroid and the largest rigid turn of a start.
 *   Start 0 is the input's bits, the identity transform and zero angles.
 *   Start s >= 1: c the atom centroid summed in atom order (as the walk forms it), q = x - c.  Philox4x32-10 with the key
 *   (seed & 0xffffffff, seed >> 32) of mcg_sampler_noise_keyed and the counter (sample_id, s, j, 0xfffffffe), j = 0..5; a
 *   word w gives the uniform u = (w >> 8) 2^-24.  j = 0: the axis (z = 2 u0 - 1, phi = 2 pi u1, (sqrt(1 - z^2) cos phi,
 *   sqrt(1 - z^2) sin phi, z)) and the angle max_turn u2.  j = 1: the shift d, its direction formed from (u0, u1) as the
 *   axis is, its length spread cbrt(u2).  j = 2..5: theta_k = 2 pi u - pi for k = 4 (j - 2) .. 4 (j - 2) + 3.  The torsions
 *   k < n_torsions are turned in ascending k on q, torsion k by theta_k about its current axis through q_b (the walk's own
 *   turn); then x_s = q' @ R_s + (c + d), R_s the walk's trial rotation of the identity by the angle about the axis.
 *   start_xyz[B,S,N,3]: the starts, 0 in padded slots; start_xform[B,S,12]: the rigid part as x' = x @ R + t (R_s, then
 *   (c + d) - c @ R_s); start_angles[B,S,16]: theta_k, 0 in unused slots; start_params[B,S,24] (may be NULL; for tests): the
 *   uniforms, draw j in columns 4 j .. 4 j + 3, zeros for start 0.
 *   A row without atoms or with a non-finite coordinate on a real atom returns every start as the input came (0 in padded
 *   slots) with NaN in xform and angles.  A result depends on (seed, sample id, s) and the row's own data only: the same
 *   bits in any batch, at any row and at any padded width.
 * MCG_ERR_ARG, nothing launched: a null buffer (start_params excepted), B outside 1..MCG_RECEPTOR_MAX_B, N outside 1..64,
 * S outside 1..MCG_SEARCH_MAX_STARTS, spread negative or not finite, max_turn outside [0, pi]. */
int mcg_pose_starts(const float* lig_xyz, const int32_t* n_nodes_dev, int B, int N, const int32_t* torsion_atoms /*[B,16,2]*/,
                    const uint64_t* side_mask /*[B,16]*/, const int32_t* n_torsions /*[B]*/,
                    const int64_t* sample_ids_dev /*[B]*/, uint64_t seed, int S, float spread, float max_turn,
                    float* start_xyz /*[B,S,N,3]*/, float* start_xform /*[B,S,12]*/, float* start_angles /*[B,S,16]*/,
                    float* start_params /*optional [B,S,24]*/, void* stream);

/* ---- The choice among the walked starts, one 64-lane wave per molecule.
 *   walk_coords[B,S,N,3], walk_xform[B,S,12], walk_stats[B,S,12], walk_angles[B,S,16]: mcg_receptor_optimise_flex's outputs
 *   for the B * S start rows; start_xform[B,S,12], start_angles[B,S,16]: mcg_pose_starts' for them; lig_xyz[B,N,3],
 *   n_nodes_dev[B]: the input of mcg_pose_starts.
 *   J_s = W_after + 0.840f CLASH_after, the product and the sum each rounded once: the walk's own acceptance quantity.  The
 *   winner is the smallest finite J; NaN and infinities never win, -0 and +0 are equal, a tie goes to the lowest s.
 *   coords_out[B,N,3]: the winner's bits.  xform_out[B,12]: the start's map followed by the walk's, R = R_s @ G_w,
 *   t = t_s @ G_w + t_w, every product rounded and summed in index order.  angles_out[B,16]: theta + the walk's summed
 *   angles.  stats_out[B,12] in mcg_receptor_optimise_flex's layout: W before and CLASH before are start 0's; W after, CLASH
 *   after, trials, kept, final s_t and torsions used the winner's; the RMSD of lig_xyz against coords_out over the real
 *   atoms; the conformer RMSD sqrt(mean |(x_out - t) @ R^T - x_in|^2).  best_start[B] int32; start_scores[B,S]: every J.
 *   Where start 0 wins, every output is start 0's walk row bit for bit.  Where no J is finite, the outputs are start 0's
 *   walk row and best_start = -1.
 * MCG_ERR_ARG, nothing launched: a null buffer, B outside 1..MCG_RECEPTOR_MAX_B, N outside 1..64, S outside
 * 1..MCG_SEARCH_MAX_STARTS. */
int mcg_pose_search_select(const float* walk_coords, const float* walk_xform, const float* walk_stats,
                           const float* walk_angles, const float* start_xform, const float* start_angles,
                           const float* lig_xyz, const int32_t* n_nodes_dev, int B, int N, int S,
                           float* coords_out /*[B,N,3]*/, float* xform_out /*[B,12]*/, float* stats_out /*[B,12]*/,
                           float* angles_out /*[B,16]*/, int32_t* best_start /*[B]*/, float* start_scores /*[B,S]*/,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
