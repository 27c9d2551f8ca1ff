/* Pockets from the receptor ("Pockets from the receptor"): the blocked-ray masks of a cubic grid of
 * points round a place on a receptor, from which the host (ml_conformer_generator_amd/pocket.py) grows the cavity and builds
 * the watertight mesh the solid-reference entries of mlconfgen_hip.h consume.  A third public header of
 * libmlconfgen_hip.so: plain C99 / C++, the conventions, error codes and stream contract of mlconfgen_hip.h, which it
 * includes for the shared limit MCG_RECEPTOR_MAX_ATOMS.  The entry returns 0 on success and MCG_ERR_ARG (1) with
 * mcg_last_error() text for an argument it refuses, before anything is enqueued.  `stream` is the hipStream_t ALL the work
 * goes to, the zeroing of the output included; nothing here synchronises, allocates or keeps state.
 * The package's OWN labelled definition, in the family of LIGSITE's and PocketPicker's buriedness: it is neither program. */
#ifndef MLCONFGEN_HIP_POCKET_H
#define MLCONFGEN_HIP_POCKET_H

#include "mlconfgen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCG_POCKET_MAX_N 127        /* grid points per axis */
#define MCG_POCKET_DIRECTIONS 26    /* rays per point: bits 0..25 of a mask */
#define MCG_POCKET_OCCUPIED 0x80000000u   /* bit 31 of a mask */
#define MCG_POCKET_MAX_SPLITS 256

/* ---- Blocked-ray masks of the n^3 points of a grid, one lane per point.
 *   Grid: point (i, j, l), 0 <= i, j, l < n, lies at ((i - c) h, (j - c) h, (l - c) h) with c = (n - 1) / 2 and h = spacing
 *   (n odd puts a point on the origin); its mask is masks[(i n + j) n + l].  The caller has moved the place of interest to
 *   the origin: every coordinate here is relative to it.
 *   rec_xyzr[R,4] fp32: (x, y, z, van der Waals radius r) per receptor atom, finite; any order - tile_sphere[ceil(R/256),4]
 *   (optional): centre and radius of a sphere that holds each run of 256 consecutive atoms with their radii; a workgroup
 *   then leaves out the runs that cannot reach its points.  Neither the order nor tile_sphere nor `splits` changes a bit.
 *   Directions: the 26 vectors (a, b, c) in {-1, 0, 1}^3 without (0, 0, 0), normalised, in lexicographic order with a
 *   slowest; direction k is bit k (direction 25 - k is minus direction k).
 *   Per point p and atom (y, r), d = y - p, all fp32, every product and sum rounded on its own:
 *     bit 31 (occupied)  iff |d|^2 < (r + probe)^2;
 *     bit k (blocked)    iff the segment {p + s u_k, 0 <= s <= reach} meets the atom's sphere: t = d . u_k,
 *                        t_c = min(max(t, 0), reach), e = d - t_c u_k componentwise, |e|^2 <= r^2.
 *   masks[n^3] uint32: the OR over all atoms; bits 26..30 are 0.  `splits`: the number of parts a workgroup's atom runs are
 *   cut into (gridDim.y); with splits > 1 the output is zeroed on `stream` first and the parts are ORed into it.
 * MCG_ERR_ARG, nothing enqueued: a null rec_xyzr or masks, n outside 1..MCG_POCKET_MAX_N, R outside
 * 1..MCG_RECEPTOR_MAX_ATOMS, spacing, probe or reach not finite or not positive, splits outside 1..MCG_POCKET_MAX_SPLITS. */
int mcg_pocket_masks(const float* rec_xyzr /*[R,4]*/, int R, const float* tile_sphere /*optional [ceil(R/256),4]*/, int n,
                     float spacing, float probe, float reach, int splits, uint32_t* masks /*[n^3]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
