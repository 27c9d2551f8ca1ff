/* Receptor contacts ("Receptor contacts"): which groups of receptor atoms - residues - a posed
 * molecule touches and with which kind of contact, and how much of a reference fingerprint it keeps.  A fifth public header
 * of libmlconfgen_hip.so: plain C99 / C++, the conventions, error codes and stream contract of mlconfgen_hip.h, which it
 * includes for the shared limits (MCG_RECEPTOR_MAX_B, MCG_RECEPTOR_MAX_ATOMS).  The entry returns 0 on success and
 * MCG_ERR_ARG (1) with mcg_last_error() text for an argument it refuses, before any launch.  `stream` is the hipStream_t
 * ALL the work goes to; nothing here synchronises, allocates or keeps state.
 * The package's OWN labelled definition (ml_conformer_generator_amd/contacts.py): it is NOT the output of ProLIF, PLIP or
 * SIFt; heavy atoms only; no ionic, aromatic or metal kinds - the type byte has no such bits. */
#ifndef MLCONFGEN_HIP_CONTACTS_H
#define MLCONFGEN_HIP_CONTACTS_H

#include "mlconfgen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MCG_CONTACT_MAX_GROUPS 256        /* entries per molecule */
#define MCG_CONTACT_MAX_CANDIDATES 2048   /* contacting receptor atoms per molecule the kernel can hold */

#define MCG_CONTACT_CONTACT 1             /* kind bits */
#define MCG_CONTACT_HYDROPHOBIC 2
#define MCG_CONTACT_HBOND_DONOR 4         /* the ligand atom donates */
#define MCG_CONTACT_HBOND_ACCEPTOR 8      /* the ligand atom accepts */
#define MCG_CONTACT_ALL_KINDS 15

#define MCG_CONTACT_OK 0                  /* status of a row */
#define MCG_CONTACT_EMPTY 1               /* no atoms: no entries */
#define MCG_CONTACT_NONFINITE 2           /* a non-finite coordinate on a real atom: no entries, counts -1 */
#define MCG_CONTACT_OVERFLOW 3            /* more than MCG_CONTACT_MAX_GROUPS groups or MCG_CONTACT_MAX_CANDIDATES receptor
                                             atoms in contact: no entries, counts -1 */

/* ---- The contact fingerprint of B posed molecules, one 256-lane workgroup per molecule.
 *   lig_xyz[B,N,3], lig_radius[B,N] (interaction radii), lig_type[B,N] (bits 1 donor, 2 acceptor, 4 hydrophobic),
 *   n_nodes_dev[B] (clamped to 0..N): as mcg_receptor_interactions takes them.  rec_xyzr[R,4] (x, y, z, interaction radius),
 *   rec_type[R], rec_group[R] int32 >= 0: the receptor's atoms, their type bits and the group - residue - each belongs to;
 *   tile_sphere[ceil(R/256),4] (optional): a sphere round each run of 256 consecutive atoms with their radii; a workgroup
 *   then walks only the runs within reach.  Neither the atoms' order nor tile_sphere changes a bit of the result.
 *   Pair (ligand atom i, receptor atom j), all fp32, every product and sum rounded on its own - the geometry of
 *   mcg_receptor_interactions: r2 = dx*dx + dy*dy + dz*dz; the pair is looked at iff r2 < 64.0f;
 *   d = sqrtf(r2) - (R_i + R_j).  It sets
 *     MCG_CONTACT_CONTACT         d <= 0.5f;
 *     MCG_CONTACT_HYDROPHOBIC     both atoms hydrophobic and d <= 0.5f;
 *     MCG_CONTACT_HBOND_DONOR     ligand atom a donor, receptor atom an acceptor, d <= -0.7f;
 *     MCG_CONTACT_HBOND_ACCEPTOR  ligand atom an acceptor, receptor atom a donor, d <= -0.7f.
 *   groups[B,256] / kinds[B,256] / n_groups[B]: per molecule the groups with kinds != 0 - kinds the OR over all pairs of the
 *   molecule's real atoms with the group's atoms - in ascending group order, zero behind the count.
 *   atom_kinds[B,N]: per ligand atom the OR of the kinds of its pairs, 0 on padded atoms.  status[B]: MCG_CONTACT_*; a row
 *   that is not OK has no entries and zero atom_kinds.
 *   counts[B,3] (optional): with it the row's entries are joined against the reference fingerprint ref_group[K_ref]
 *   (ascending, no group twice) / ref_kinds[K_ref] over the bits of kinds_mask: n_bits (the row's), n_ref_bits (the
 *   reference's), n_common (set in both) - exact integers; -1, -1, -1 on a NONFINITE or OVERFLOW row.  Without counts the
 *   three reference arguments are not read.
 *   No atomics; a row's outputs depend on its own atoms and the receptor arrays only.
 * MCG_ERR_ARG, nothing launched: a null buffer (tile_sphere and counts excepted; ref_group and ref_kinds only with counts and
 * K_ref > 0), B outside 1..MCG_RECEPTOR_MAX_B, N outside 1..64, R outside 1..MCG_RECEPTOR_MAX_ATOMS, K_ref outside
 * 0..MCG_CONTACT_MAX_GROUPS, kinds_mask outside 0..MCG_CONTACT_ALL_KINDS. */
int mcg_receptor_contacts(const float* lig_xyz /*[B,N,3]*/, const float* lig_radius /*[B,N]*/,
                          const uint8_t* lig_type /*[B,N]*/, const int32_t* n_nodes_dev /*[B]*/, int B, int N,
                          const float* rec_xyzr /*[R,4]*/, const uint8_t* rec_type /*[R]*/,
                          const int32_t* rec_group /*[R]*/, int R, const float* tile_sphere /*optional*/,
                          const int32_t* ref_group /*[K_ref]*/, const uint8_t* ref_kinds /*[K_ref]*/, int K_ref,
                          int kinds_mask, int32_t* groups /*[B,256]*/, uint8_t* kinds /*[B,256]*/,
                          int32_t* n_groups /*[B]*/, uint8_t* atom_kinds /*[B,N]*/, int32_t* status /*[B]*/,
                          int32_t* counts /*optional [B,3]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
