"""The coverage table of tests/stream_probe.py held against include/mlconfgen_hip.h: an entry point that takes a stream cannot
land without a stream test (tests/test_stream_contract_gpu.py).  No GPU is needed."""
import os
import re

import stream_probe as P

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOWED_EXCLUSIONS = {"mcg_debug_gemm", "mcg_bench_edge", "mcg_bench_edge_incall", "mcg_egnn_gcl_debug", "mcg_egnn_gcl_debug_ex",
                      "mcg_egnn_block_debug", "mcg_egnn_equiv_debug"}


def test_the_header_parse_finds_the_stream_taking_prototypes():
    names = P.stream_entries()
    assert len(names) == len(set(names)) >= 50, names
    for known in ("mcg_egnn_dynamics", "mcg_sampler_noise_keyed", "mcg_gcn_forward", "mcg_shape_overlay_refined",
                  "mcg_receptor_optimise", "mcg_debug_gemm", "mcg_handoff"):
        assert known in names, known
    for no_stream in ("mcg_gcn_check", "mcg_plan_create_ex", "mcg_debug_route", "mcg_mesh_splits", "mcg_last_error"):
        assert no_stream not in names, no_stream


def test_every_stream_taking_entry_is_in_the_table_or_excluded_with_a_reason():
    missing = [n for n in P.stream_entries() if n not in P.COVERAGE and n not in P.ALIASES and n not in P.EXCLUDED]
    assert not missing, f"entry points that take a stream and have no stream test: {missing}"
    assert set(P.EXCLUDED) <= ALLOWED_EXCLUSIONS, sorted(set(P.EXCLUDED) - ALLOWED_EXCLUSIONS)
    assert all(isinstance(why, str) and len(why) > 20 for why in P.EXCLUDED.values())
    assert not set(P.EXCLUDED) & set(P.COVERAGE) and not set(P.ALIASES) & (set(P.COVERAGE) | set(P.EXCLUDED))
    for alias, target in P.ALIASES.items():
        assert target in P.COVERAGE, (alias, target)


def test_every_table_key_is_a_declared_entry_that_takes_a_stream():
    from ml_conformer_generator_amd import _lib
    takes_stream = set(P.stream_entries())
    for name in list(P.COVERAGE) + list(P.ALIASES) + list(P.EXCLUDED):
        assert name in _lib.SIGNATURES, name
        assert name in takes_stream, name


def test_every_table_entry_names_its_gpu_test_and_its_arrangements():
    with open(os.path.join(HERE, "test_stream_contract_gpu.py")) as f:
        source = f.read()
    tests = set(re.findall(r"^def (test_\w+)\(", source, flags=re.M))
    for name, (test, arrangements, why_only_a) in P.COVERAGE.items():
        assert test in tests, (name, test)
        assert f'claims("{test}")' in source, test             # the GPU test checks that it ran what the table gives it
        assert arrangements in ("A", "AB"), (name, arrangements)
        assert (why_only_a is None) == (arrangements == "AB"), name
        assert why_only_a is None or len(why_only_a) > 20, name
