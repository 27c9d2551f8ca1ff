/* Flexible pose ("Flexible pose"): the torsion tree of a heavy-atom graph and the walk that turns its
 * rotatable bonds beside the rigid-body move of mcg_receptor_optimise.  A second public header of libmlconfgen_hip.so: plain
 * C99 / C++, the conventions, error codes and stream contract of mlconfgen_hip.h, which it includes for the shared limits
 * (MCG_RECEPTOR_MAX_B, MCG_RECEPTOR_MAX_ATOMS).  Every entry returns 0 on success and MCG_ERR_ARG (1) with
 * mcg_last_error() text for an argument it refuses, before any launch.  `stream` is the hipStream_t the work goes to;
 * nothing here synchronises, allocates or keeps state.
 * The package's OWN procedure: not a docking run, not AutoDock Vina's optimiser, no global search. */
#ifndef MLCONFGEN_HIP_FLEX_H
#define MLCONFGEN_HIP_FLEX_H

#include "mlconfgen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCG_FLEX_MAX_ATOMS 64     /* atoms per molecule: one lane, one bit of a 64-bit mask */
#define MCG_FLEX_MAX_TORSIONS 16  /* torsions used per molecule; more are counted and stay frozen */
#define MCG_FLEX_MAX_B 16384
#define MCG_FLEX_STATS 12         /* columns of stats_out */
#define MCG_FLEX_GRADIENT 22      /* columns of gradient_out: F[3], torque[3], tau[16] */
#define MCG_FLEX_TRACE 43         /* columns of trace_out */

/* ---- The torsion tree of B heavy-atom graphs, one 64-lane wave per molecule, lane = atom.  Integer work only: exact, the
 * same bits in any batch, at any row and at any padded width.
 *   z[B,W] int32 atomic numbers, bonds[B,W,W] int8 symmetric codes 0 / 1 / 2 / 3 / 4 (the diagonal, everything at or beyond
 *   n_nodes_dev[b] and every other code are read as 0), n_nodes_dev[B] clamped to 0..W.
 *   A torsion is a code-1 bond that is no ring bond (reachable round the bond left out) whose two ends both have heavy
 *   degree >= 2, unless it joins a nitrogen to a carbon that has a code-2 bond to N, O or S (amide, urea, carbamate).
 *   Leaving the bond out splits its component in two; the MOVING side is the part with fewer atoms, on a tie the part
 *   that holds the bond's higher-indexed end.  Torsions in ascending (min, max) order of their ends; the first
 *   MCG_FLEX_MAX_TORSIONS are written.
 *   torsion_atoms[B,16,2] int32: per torsion (a, b), b the end inside the moving side; (-1, -1) in unused slots.
 *   side_mask[B,16] uint64: bit i set iff atom i is in the moving side (b included); 0 in unused slots.
 *   near_mask[B,W] uint64: bit j of entry i set iff j is i, a bonded neighbour of i or shares a bonded neighbour with i;
 *   0 at and beyond the row's atoms.
 *   counts[B,2] int32: torsions found, torsions used (= min(found, 16)).
 * B = 0 launches nothing.  MCG_ERR_ARG, nothing launched: a null buffer, B outside 0..MCG_FLEX_MAX_B, W outside
 * 1..MCG_FLEX_MAX_ATOMS. */
int mcg_torsion_tree(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                     int32_t* torsion_atoms /*[B,16,2]*/, uint64_t* side_mask /*[B,16]*/, uint64_t* near_mask /*[B,W]*/,
                     int32_t* counts /*[B,2]*/, void* stream);

/* ---- Flexible pose: mcg_receptor_optimise's walk with the torsions of mcg_torsion_tree turned beside the rigid move and
 * an intramolecular guard.  One 256-lane workgroup per molecule in that entry's layout; the receptor loop, the pair
 * arithmetic, the tile list and the rigid trial are its shared text.
 *   lig_xyz .. max_shift: as for mcg_receptor_optimise.  clash_radius[B,N]: c_i (covalent radius + 0.45 A).
 *   torsion_atoms, side_mask, near_mask (width N): mcg_torsion_tree's outputs for the same rows; n_torsions[B] the torsions
 *   to use, clamped to 0..16 and cut at the first slot whose atoms are not inside the row.
 *   State (q, G, p) from q_i = x_i - c, G = I, p = c; world x_i = q_i @ G + p.  CLASH = sum over real pairs i < j with j not
 *   in near[i] of max(0, (c_i + c_j) - |q_i - q_j|)^2, always from q.  One evaluation: the five term sums, F and the torque
 *   about p as mcg_receptor_optimise forms them, CLASH, and per torsion tau_k = n_k . sum_{i in side_k} (x_i - x_b) x f_i,
 *   n_k the unit vector from a to b, f_i the receptor force on i plus 0.840 times its clash force rotated into the world
 *   frame.  A trial turns torsion k = 0, 1, ... of a copy of q by s_tau tau_k / max_j |tau_j| about its current axis
 *   through q_b (a zero angle leaves the bits), then rotates by s_r about the torque and moves p by s_t along F.  A zero
 *   or non-finite vector skips its part; all three skipped ends the walk.  From s_r = 0.05, s_t = 0.25, s_tau = 0.1; kept:
 *   all x 1.2, rejected: x 0.5; ends after `steps` trials or once s_t < 2^-8.  Rejected unevaluated: |p' - c| > max_shift
 *   or any |q'_i| > rho0 + 2, rho0 the largest |x_i - c| of the input.  Kept iff (W' - W) + 0.840f (C' - C) < 0 in fp32.
 *   A row without a torsion returns mcg_receptor_optimise's bits.
 *   coords_out[B,N,3]; xform_out[B,12]: the rigid part (G, p) as x' = x @ R + t; stats_out[B,12]: W before, W after,
 *   trials, kept, heavy-atom RMSD input to output, final s_t, CLASH before, CLASH after, torsions used, conformer RMSD (q at
 *   the end against q at the start), 0, 0; angles_out[B,16]: the summed kept angles; gradient_out[B,22] (may be NULL): F,
 *   torque, tau at the input; trace_out[B,steps,43] (may be NULL; for tests): mcg_receptor_optimise's 24 columns, then
 *   s_tau, tau[16] and C of the current state, C' of the trial (0 where not evaluated); rows beyond the last trial zero.
 *   A molecule without atoms or with a non-finite coordinate on a real atom returns its rows as they came and NaN in
 *   xform, stats, angles and gradient (trace rows zero); the others are unaffected.
 * MCG_ERR_ARG, nothing launched: a null buffer (tile_sphere, gradient_out, trace_out excepted), B outside
 * 1..MCG_RECEPTOR_MAX_B, N outside 1..64, R outside 1..MCG_RECEPTOR_MAX_ATOMS, steps outside 0..1024, max_shift negative or
 * not finite. */
int mcg_receptor_optimise_flex(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                               const int32_t* n_nodes_dev, int B, int N, const float* rec_xyzr, const uint8_t* rec_type,
                               int R, const float* tile_sphere /*optional*/, int steps, float max_shift,
                               const float* clash_radius /*[B,N]*/, const int32_t* torsion_atoms /*[B,16,2]*/,
                               const uint64_t* side_mask /*[B,16]*/, const uint64_t* near_mask /*[B,N]*/,
                               const int32_t* n_torsions /*[B]*/, float* coords_out /*[B,N,3]*/,
                               float* xform_out /*[B,12]*/, float* stats_out /*[B,12]*/, float* angles_out /*[B,16]*/,
                               float* gradient_out /*optional [B,22]*/, float* trace_out /*optional [B,steps,43]*/,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
