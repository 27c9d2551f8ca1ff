// Internal glue between the translation units of libmlconfgen_hip.so.
#pragma once
#include "../../include/mlconfgen_hip.h"

#include <stddef.h>

// accessors of the opaque plan (defined in mcg_egnn_plan.hip)
int mcg_plan_B(const mcg_plan* p);
int mcg_plan_N(const mcg_plan* p);
const int* mcg_plan_n_nodes(const mcg_plan* p);   // device pointer
// "everything enqueued on this plan so far" -> the plan's completion event, recorded on the caller's stream
// (mcg_plan_destroy waits for it before the plan's blocks return to the pool)
void mcg_plan_mark_done(const mcg_plan* p, void* stream);

// device-memory pool of the handles' workspaces (mcg_devmem.hip): freed blocks are kept and handed out again, so neither
// call reaches the driver in steady state - and mcg_dev_free, unlike hipFree, does not wait for the device: the caller
// guarantees that nothing still runs on the block
int mcg_dev_alloc(size_t bytes, void** out);
void mcg_dev_free(void* p);
void mcg_dev_trim();

// mcg_shape_overlay behind both overlay entries (mcg_shape.hip): checks its arguments and the calling entry's own
// conditions `more_ok` (the message names `who` and ends with `more`), then launches k_shape_density and k_shape_overlay.
int mcg_shape_overlay_launch(const char* who, bool more_ok, const char* more, const float* ref_frame, int n_ref,
                             const float* ref_xform, const float* frames, const float* xform, const int32_t* n_nodes_dev,
                             int B, int N, const float* rot, const float* axes, int n, float alpha, float amplitude,
                             float* f_scratch, float* score, float* best, int32_t* which, int32_t* flipped, float* pose,
                             float* posed, void* stream);
