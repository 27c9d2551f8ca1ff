"""ctypes binding of libmlconfgen_hip.so (the C ABI in include/mlconfgen_hip.h).

The library is the product: if it is missing or does not export a declared
symbol, importing this module's `lib()` raises - there is no CPU/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCG_LIB_PATH: measurement builds only (tools/build_variants.sh: ablation / experiment variants of the same library)
LIB_PATH = os.environ.get("MCG_LIB_PATH") or os.path.join(_HERE, "libmlconfgen_hip.so")

_vp, _i, _f, _d = C.c_void_p, C.c_int, C.c_float, C.c_double
_pp = C.POINTER(C.c_void_p)

# name -> (restype, argtypes); mirrors include/mlconfgen_hip.h one to one
SIGNATURES: Dict[str, tuple] = {
    "mcg_last_error": (C.c_char_p, []),
    "mcg_abi_version": (_i, []),
    "mcg_egnn_create": (_i, [_pp, _i, _i, _i, _pp]),
    "mcg_egnn_destroy": (None, [_vp]),
    "mcg_egnn_set_precision": (_i, [_vp, _i]),
    "mcg_egnn_set_option": (_i, [_vp, _i, _i]),
    "mcg_debug_gemm_launches": (_i, [_vp, _i]),
    "mcg_debug_gemm": (_i, [_vp, _vp, _vp]),
    "mcg_debug_gemm_pack": (_i, [_vp, _i, _i, _i, _i, _vp, C.c_int64, _vp]),
    "mcg_plan_create": (_i, [_i, _i, _vp, _i, _pp]),
    "mcg_plan_create_ex": (_i, [_i, _i, _vp, _vp, _pp]),
    "mcg_plan_destroy": (None, [_vp]),
    "mcg_pool_stats": (_i, [_vp, _i]),
    "mcg_plan_info": (_i, [_vp, _vp]),
    "mcg_plan_ranges": (_i, [_vp]),
    "mcg_plan_set_latency_mode": (_i, [_vp, _i]),
    "mcg_plan_check_tables": (_i, [_i, _i, _vp, _vp, _i, _vp]),
    "mcg_egnn_dynamics": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_egnn_block_debug": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mcg_egnn_gcl_debug": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mcg_plan_peek": (_i, [_vp, _i, _vp, _vp]),
    "mcg_egnn_gcl_debug_ex": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "mcg_egnn_equiv_debug": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "mcg_debug_route": (_i, [_vp, _vp, _i, _vp]),
    "mcg_bench_edge": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "mcg_bench_edge_incall": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "mcg_sampler_noise": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mcg_sampler_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp]),
    "mcg_sampler_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "mcg_sampler_blend": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _vp]),
    "mcg_sampler_noise_keyed": (_i, [_vp, C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "mcg_egnn_aggregate": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "mcg_gcn_create": (_i, [_pp, _i, _pp]),
    "mcg_gcn_destroy": (None, [_vp]),
    "mcg_gcn_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mcg_gcn_check": (_i, [_vp]),
    "mcg_gcn_peek": (_i, [_vp, _i, _i, _vp, _vp]),
    "mcg_shape_tanimoto": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _f, _f, _vp, _vp, _vp]),
    "mcg_shape_moments": (_i, [_vp, _vp, _i, _i, _d, _d, _f, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_shape_frames": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _d, _d, _f, _i, _i, _vp, _vp, _vp]),
    "mcg_shape_frames_tf": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _d, _d, _f, _i, _i, _vp, _vp, _vp, _vp]),
    "mcg_shape_overlay": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp]),
    "mcg_shape_overlay_refined": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_shape_pair_tanimoto": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp]),
    "mcg_receptor_overlap": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mcg_receptor_relieve": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "mcg_receptor_interactions": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_receptor_optimise": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_graph_fingerprint": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "mcg_fingerprint_tanimoto": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mcg_fingerprint_pair_tanimoto": (_i, [_vp, _i, _vp, _vp]),
    "mcg_mesh_splits": (_i, [_i]),
    "mcg_mesh_winding": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "mcg_mesh_occupancy": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp]),
    "mcg_mesh_atoms_outside": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mcg_shape_tanimoto_field": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _f, _f, _vp, _vp]),
    "mcg_shape_overlay_field": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp]),
    "mcg_geometry_relax": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_geometry_relax_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_pharm_perceive": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "mcg_pharm_score": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_hydrogens_place": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_standardize_graphs": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_charges_peoe": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_esp_overlap": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "mcg_canonical_order": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_stereo_order": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_substructure_match": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_ring_scaffold": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_induced_subgraph": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_handoff": (_i, [_vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "mcg_handoff_ex": (_i, [_vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_handoff_elements": (_i, [_vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcg_bond_writeback": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "mcg_ifm_merge": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/mlconfgen_hip_flex.h one to one (a second public header: DESIGN.md section 6,
# "Flexible pose")
FLEX_SIGNATURES: Dict[str, tuple] = {
    "mcg_torsion_tree": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcg_receptor_optimise_flex": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/mlconfgen_hip_pocket.h one to one (a third public header: DESIGN.md section 6,
# "Pockets from the receptor")
POCKET_SIGNATURES: Dict[str, tuple] = {
    "mcg_pocket_masks": (_i, [_vp, _i, _vp, _i, _f, _f, _f, _i, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/mlconfgen_hip_search.h one to one (a fourth public header: DESIGN.md section 6,
# "Pose search")
SEARCH_SIGNATURES: Dict[str, tuple] = {
    "mcg_pose_starts": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, C.c_uint64, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "mcg_pose_search_select": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/mlconfgen_hip_contacts.h one to one (a fifth public header: DESIGN.md section 6,
# "Receptor contacts")
CONTACT_SIGNATURES: Dict[str, tuple] = {
    "mcg_receptor_contacts": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp]),
}


class PlanOpts(C.Structure):
    """`mcg_plan_opts` (include/mlconfgen_hip.h): zero-initialised = the library's defaults."""
    _fields_ = [("edge_mt", C.c_int32), ("n_ranges", C.c_int32), ("four_tile_units", C.c_int32), ("reserved", C.c_int32 * 5)]


class GemmDesc(C.Structure):
    """`mcg_gemm_desc` (include/mlconfgen_hip.h): one node-GEMM launch of `mcg_debug_gemm`; zero-initialised = unused."""
    _fields_ = ([(n, C.c_void_p) for n in ("A1", "A2", "bias", "resid", "C", "a2_rows", "side_u", "side_slots", "side_x", "w_host")]
                + [(n, C.c_int64) for n in ("a1_floats", "a2_floats", "resid_floats", "c_floats")]
                + [(n, C.c_int32) for n in ("lda1", "lda2", "ldr", "ldc", "M", "K1", "K2", "n_out", "n_store", "act", "a2_nsum",
                                            "a2_src_rows", "side_M", "side_u_rows", "c_blocked", "family", "rn", "mr", "deep", "lds")]
                + [("reserved", C.c_int32 * 4)])


class GemmRan(C.Structure):
    """`mcg_gemm_ran`: the kernel template (GEMM_KERNEL_*) and template arguments `mcg_debug_gemm` ran."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "rn", "mr", "ring", "gather", "resid", "seg2", "reserved")]


GEMM_F32, GEMM_F32ROWS16, GEMM_BF16, GEMM_X6 = 0, 1, 2, 3                    # mcg_gemm_desc.family
GEMM_KERNEL_F32, GEMM_KERNEL_F32ROWS16, GEMM_KERNEL_BF16, GEMM_KERNEL_BF16_LDS, GEMM_KERNEL_X6 = 1, 2, 3, 4, 5
GEMM_PACK4, GEMM_PACK16, GEMM_PACK16X3 = 0, 1, 2
ALL_FOUR_TILE = 0x3fffffff          # MCG_ALL_FOUR_TILE
OPT_X6_GEMM, OPT_GEMM_RN, OPT_GEMM_X6_RN, OPT_GEMM_BF16_LDS, OPT_NODE_FUSED = 1, 2, 3, 4, 5

# mcg_debug_route: info[0] edge kernel, info[2] aggregate source, info[5] coordinate update (info[1] / info[4]: GEMM_* families)
ROUTE_EDGE = ("Exact", "Ns", "Bf16Rows16", "W64Bf16", "W64X6", "Invalid")
ROUTE_GEMM = ("F32", "F32Rows16", "Bf16", "X6")
ROUTE_AGG = ("GatherU", "GatherP", "GatherAgg2", "Combine")
ROUTE_COORD = ("PendingU", "PendingP", "Kernel")

_lib = None


class McgError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raise if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise McgError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ml_conformer_generator_amd/csrc`. There is no CPU fallback for the hot path.")
    import torch  # noqa: F401  - loads the process's HIP runtime first (same SONAME as ours)
    handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in (list(SIGNATURES.items()) + list(FLEX_SIGNATURES.items()) + list(POCKET_SIGNATURES.items())
                              + list(SEARCH_SIGNATURES.items()) + list(CONTACT_SIGNATURES.items())):
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise McgError(f"{LIB_PATH} does not export `{name}` (stale build?)") from e
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return handle


def debug_route(model_handle, plan_handle, keep_agg: bool = False) -> dict:
    """`mcg_debug_route` by name: what the library's routing function decides for this model and plan (no launch)."""
    info = (C.c_int32 * 8)()
    check(lib().mcg_debug_route(model_handle, plan_handle, 1 if keep_agg else 0, info), "mcg_debug_route")
    return {"edge": ROUTE_EDGE[info[0]], "pab": ROUTE_GEMM[info[1]], "agg": ROUTE_AGG[info[2]], "fused": bool(info[3]),
            "node": ROUTE_GEMM[info[4]], "coord": ROUTE_COORD[info[5]], "pspan": int(info[6]), "unit_span": int(info[7])}


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().mcg_last_error()
        raise McgError(f"{what} failed (code {code}): {msg.decode() if msg else ''}")


def host_ptr_array(tensors: Sequence) -> "C.Array":
    """void*[n] of HOST data pointers of contiguous fp32 CPU tensors."""
    arr = (C.c_void_p * len(tensors))()
    for k, t in enumerate(tensors):
        assert t.device.type == "cpu" and t.is_contiguous() and str(t.dtype) == "torch.float32"
        arr[k] = t.data_ptr()
    return arr


def dptr(t) -> int:
    """Device (or host) data pointer of a contiguous tensor, as int for ctypes."""
    if t is None:
        return None
    assert t.is_contiguous(), "kernel operands must be contiguous"
    return t.data_ptr()


def current_stream_ptr(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream
