"""The rounding model of the bf16 operand mode (tests/bf16_ref.py) on the CPU: anchored to the oracle, with room for its own
fp32 evaluation under the acceptance rule the GPU module (tests/test_bf16_stages_gpu.py) uses, and able to see the mistakes a
kernel of this mode can make - wrong rounding point, lost k-tail, lost edge, lost partial row."""
import pytest
import torch

import bf16_cases as Cs
import bf16_ref as R

ROOM = 4.0


def dense_view(shape):
    """The shape's compact inputs as the dense [B * N] arrays the oracle takes, and the mask of the real slots."""
    from oracle import egnn_oracle as EO
    from oracle import host_oracle as HO
    geo, h, x, x0 = Cs.inputs(shape)
    sizes = torch.tensor(geo.sizes)
    N = int(sizes.max())
    nm, em = HO.masks_from_sizes(sizes, N)
    real = nm.reshape(-1) > 0
    B = len(geo.sizes)

    def dense(a):
        out = torch.zeros(B * N, a.shape[1], dtype=torch.float64)
        out[real] = a.double()
        return out
    row, col = EO.dense_edge_index(N, B)
    return dense(h), dense(x), dense(x0), row, col, nm.reshape(B * N, 1).double(), em.double(), real


@pytest.mark.parametrize("shape", ["a", "b", "d"])
def test_identity_rounding_and_exact_aggregate_is_the_oracle(shape):
    """Anchor: with identity rounding and the unrounded aggregate every stage in fp64 is oracle.egnn_oracle.gcl /
    equivariant_update in fp64, up to fp64 re-association (1e-12 of the stage's scale)."""
    from oracle import egnn_oracle as EO
    f64 = torch.float64
    sd = {k: v.double() for k, v in Cs.weights().items()}
    geo, h, x, x0 = Cs.inputs(shape)
    hd, xd, x0d, row, col, nm, em, real = dense_view(shape)
    d0, _ = EO.pair_geometry(x0d, row, col)
    d1, unit = EO.pair_geometry(xd, row, col)
    ea = torch.cat([d1, d0], 1)
    h_ref, _, _, agg_ref = EO.gcl(sd, Cs.P_GCL, hd, row, col, ea, nm, em)
    x_ref = EO.equivariant_update(sd, Cs.P_EQ, hd, xd, row, col, unit, ea, nm, em)
    g = R.gcl_stages(geo, h.double(), x.double(), x0.double(), Cs.layer(Cs.P_GCL, f64), R.identity, False)
    e = R.equiv_stages(geo, h.double(), x.double(), x0.double(), Cs.layer(Cs.P_EQ, f64), R.identity)
    w1, b1 = sd[Cs.P_GCL + "edge_mlp.0.weight"], sd[Cs.P_GCL + "edge_mlp.0.bias"]
    pab_ref = torch.cat([hd @ w1[:, :420].T + b1, hd @ w1[:, 420:840].T], 1)
    hid_ref = torch.nn.functional.silu(torch.nn.functional.linear(torch.cat([hd, agg_ref], 1), sd[Cs.P_GCL + "node_mlp.0.weight"],
                                                                  sd[Cs.P_GCL + "node_mlp.0.bias"]))
    for what, a, b in (("pab", g["pab"], pab_ref[real]), ("agg", g["agg"], agg_ref[real]), ("hidden", g["hidden"], hid_ref[real]),
                       ("h", g["h"], h_ref[real]), ("x", e["x"], x_ref[real])):
        err = float((a - b).abs().max()) / float(b.abs().max())
        assert err <= 1e-12, (shape, what, err)
    if shape == "b":          # the one-atom molecule has no edges: its aggregate is exactly zero, its coordinates do not move
        v = sum(geo.sizes[:3])
        assert geo.sizes[3] == 1 and float(g["agg"][v].abs().max()) == 0.0 and torch.equal(e["x"][v], x[v].double())


@pytest.mark.parametrize("shape", sorted(Cs.SHAPES))
def test_the_fp32_restatement_has_four_times_the_room_it_needs(shape):
    """Reference alone: the fp32 evaluation against the fp64 one, teacher-forced, under the acceptance rule with 4 x room:
    strict stages at a quarter of the tight tier on every element; flip stages with at most 0.5 % of their elements outside it
    (the outer tier and the rms bound are multiples of these very figures: their room is the factor itself)."""
    for stage, f in Cs.reference_alone(shape).items():
        print(f"\nBF16-STAGES ref-alone {shape} {stage}: {R.figures_text(f)}")
        if stage in R.FLIP_STAGES:
            assert f["share"] * ROOM <= R.FLIP_SHARE, (shape, stage, f)
        else:
            assert f["viol"] * ROOM <= 1.0, (shape, stage, f)


def test_span_and_geometry_of_the_shapes():
    """What each shape is there to reach, checked on the host as large_molecule_cases.span64 does it."""
    from large_molecule_cases import span16, span64
    for name, c in Cs.SHAPES.items():
        geo = Cs.inputs(name)[0]
        Ru = Cs.rows_per_unit(name)
        assert geo.span(Ru) == (span64 if Ru == 64 else span16)(c["sizes"]), name
        assert geo.E == sum(n * (n - 1) for n in c["sizes"])
    assert Cs.inputs("a")[0].E == 2310 and (2310 + 63) // 64 == 37 and Cs.inputs("a")[0].span(64) <= 2
    assert Cs.inputs("b")[0].E == 760 and 1 in Cs.SHAPES["b"]["sizes"] and min(Cs.SHAPES["b"]["sizes"]) < 6
    assert Cs.inputs("d")[0].E == 4902 and Cs.inputs("d")[0].span(64) == 3
    assert Cs.inputs("e")[0].span(64) >= 5
    assert Cs.inputs("f33")[0].M % 32 == 1 and Cs.inputs("f31")[0].M % 32 == 31


def test_unblock_pab_inverts_the_piece_major_store_address():
    """The helper against the store address of mcg_gemm_c_ptr (csrc/mcg_gemm_kernels.h:18-22) written out element by element."""
    M = 37
    row_major = torch.arange(M * 864, dtype=torch.float32).reshape(M, 864)
    raw = torch.zeros(M * R.PAB_BLOCKED_FLOATS)
    for nt in range(54):
        part, ntp = (1, nt - 27) if nt >= 27 else (0, nt)
        for g in range(4):
            base = ((part * 14 + (ntp >> 1)) * 8 + (ntp & 1) * 4 + g) * M
            for r in range(M):
                raw[(base + r) * 4:(base + r) * 4 + 4] = row_major[r, nt * 16 + 4 * g:nt * 16 + 4 * g + 4]
    pab, pad = R.unblock_pab(raw, M)
    assert torch.equal(pab, torch.cat([row_major[:, :420], row_major[:, 432:852]], 1))
    pab2, _ = R.rowmajor_pab(row_major, M)
    assert torch.equal(pab2, pab)
    # the last k-block of the Pb part lies beyond M * 864 floats: a row-major-sized copy of the buffer misses columns 416..419
    assert ((1 * 14 + 13) * 8) * M * 4 == M * 864


@pytest.mark.parametrize("shape", ["a", "c"])
def test_every_required_mutation_breaks_the_rule_tenfold(shape):
    """Shape (a) carries the rounded-aggregate model of the 64-row kernel, shape (c) the exact aggregate of the 16-row kernel.
    Every class's rms bound stays at or below a fifth of the least visible required mutation scored in that class.
    (`python tools/parity_sensitivity.py --bf16-stages` prints the same tables: profiles/bf16_stage_sensitivity.txt.)"""
    text = Cs.table_text(shape)
    for label, stage, required, fig, excess in Cs.mutation_table(shape):
        if required:
            assert excess >= 10.0, (label, stage, excess, fig)
    for k, least in Cs.least_visible(shape).items():
        assert R.RMS_BOUND[k] <= least / 5, (k, R.RMS_BOUND[k], least)
    assert "BLIND" not in text and text.count("(informational)") == 1
    # informational: A left unrounded in the COORDINATE layer - x' = x + update / 100 and the rounding of A moves the update by
    # 1e-3 of itself, 1e-5 of max|x'|: inside the tight tier by construction; the same rounding point is required on the aggregate


def test_the_two_aggregate_models_are_told_apart_on_every_bf16_shape():
    """The rounded aggregate scored against the exact-aggregate model, and the other way round, fails the rule on every shape
    whose kernel has either: the pin separates the two arithmetics."""
    for shape, c in Cs.SHAPES.items():
        if c["mode"] != "bf16":
            continue
        bufs = Cs.free_run(shape, torch.float32)
        own64 = Cs.forced(shape, bufs, torch.float64, ("agg",))["agg"]
        other64 = Cs.forced(shape, bufs, torch.float64, ("agg",), rounded=not c["rounded"])["agg"]
        other32 = Cs.forced(shape, bufs, torch.float32, ("agg",), rounded=not c["rounded"])["agg"]
        fig = R.judge(own64, other64, other32)
        assert not R.accepted(fig, False), (shape, fig)
        assert R.excess(fig, False) >= 10.0, (shape, fig)
