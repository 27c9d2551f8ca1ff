// What the two receptor pose walks - `k_receptor_optimise` (mcg_pose_optimise.hip) and `k_receptor_optimise_flex`
// (mcg_pose_flex.hip) - state once ("Shared device text"): the step constants and the argument check
// of their entries.  The walk's device text itself stays in each kernel file: written as one `template <bool FLEX>` body
// it kept every output bit and both resource envelopes but not the kernels' times (profiles/pose_walk_share_time.txt), so
// the flexible kernel's receptor loop, combine, trial and epilogue remain the rigid kernel's text, kept in step by hand and
// pinned from both sides by tests/test_pose_flex_gpu.py.
#pragma once

#include <math.h>

#include "mcg_api_internal.h"
#include "mcg_rigid_step.h"
#include "mcg_shape_grid.h"

namespace mcg_receptor_walk {

constexpr float RW_STEP_ROT = 0.05f;          // initial rotation step, rad
constexpr float RW_STEP_TRANS = 0.25f;        // initial translation step, Angstrom
constexpr float RW_MIN_TRANS = 0.00390625f;   // 2^-8 A: the walk ends below it
constexpr float FX_STEP_TAU = 0.1f;           // initial torsion step, rad (the torsion with the largest |tau| turns by it)
constexpr float FX_MARGIN = 2.0f;             // an atom may leave the input's radius about p by this much, Angstrom

// The checks both entries share; `buffers`: every pointer the entry requires is non-null.  Refused: the entry's message is
// set and false comes back.
inline bool walk_args_ok(const char* entry, bool buffers, int B, int N, int R, int steps, float max_shift) {
    static_assert(mcg_rigid::WALK_MAX_STEPS == 1024 && mcg_shape::MAX_ATOMS == 64, "the bounds the message below states");
    if (buffers && B >= 1 && B <= MCG_RECEPTOR_MAX_B && N >= 1 && N <= mcg_shape::MAX_ATOMS && R >= 1 &&
        R <= MCG_RECEPTOR_MAX_ATOMS && steps >= 0 && steps <= mcg_rigid::WALK_MAX_STEPS && max_shift >= 0.f &&
        isfinite(max_shift))
        return true;
    mcg_set_error("%s: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= 64, 1 <= R <= %d, 0 <= steps <= 1024, "
                  "max_shift finite and >= 0)", entry, MCG_RECEPTOR_MAX_B, MCG_RECEPTOR_MAX_ATOMS);
    return false;
}

}  // namespace mcg_receptor_walk
