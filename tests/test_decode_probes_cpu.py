"""Self-test of the persistent-decode probes (tests/decode_probes.py), on the CPU.

For every case the GPU module runs:
  * the emulation of the step, organised by the mirror of the kernel's work partition, passes the
    comparators against the plain fp64 reference, so a GPU failure is the kernel's (or the
    mirror's, which the GPU module checks against the launcher);
  * the builder's promises hold on the fp64 reference: ledger values are bf16 integers, the needle
    leads by at least 200 (log2 units), x is +-g whatever the last bit of rstd, silu(g) = g in fp32.
Every mutation of the emulation — a lost, doubled, stale or shifted weight piece, a lost or
misplaced row, a lost token, chunk or block, the wrong head, layer, table or sequence, a misplaced
append, a layer that reuses its predecessor's weights — is rejected at every case where it changes
anything the GPU test reads, and changes something at one case at least.  The two demonstrations at
the end show what the model tests' assert_close(atol=0.1, rtol=0.05) on random weights lets through.

Mutations run where they can strike.  Attention mutations run at every needle and count case.  A
weight stream never sees the context, so weight-stream and layer mutations run at one exact case of
every launch shape in the list (geometry, batch, grid, depth, which phases are on): the 67 cases that
vary the context and the target at one shape stand behind their first.
"""
import functools

import pytest
import torch

from tests import attention_probes as ap
from tests import decode_probes as dp

IDS = [c.name for c in dp.CASES]


@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(inputs, fp64 reference, bf16-emulating reference, unbroken emulation) of a case."""
    inp = dp.build(dp.case_by_name(name))
    want, emu = dp.expected(inp)
    clean, applied = dp.step(inp, "emu")
    assert not applied
    return inp, want, emu, clean


@pytest.mark.parametrize("name", IDS)
def test_unbroken_emulation_passes(name):
    inp, want, emu, clean = _prepared(name)
    case = inp.case
    assert not dp.refuses(case.geo, case.B, case.cap)
    dp.check(inp, clean, want, emu)
    if case.family == "needle":
        assert want["needle_gap"] >= 200      # dp.expected asserts it too, for every launch
        assert torch.equal(clean["attn"], want["attn"])
    # hygiene: poison in block 0 and past the contexts, scrambled tables, K / V unlike per layer and head
    assert (inp.k_cache[:, 0] == dp.POISON).all() and (inp.v_cache[:, 0] == dp.POISON).all()
    for b, n in enumerate(case.ncached):
        if n >= 0 and (n + 1) % dp.KBS:
            blk = int(inp.bt[b, n // dp.KBS])
            assert (inp.k_cache[:, blk, :, n % dp.KBS:] == dp.POISON).all()
            assert (inp.v_cache[:, blk, :, :, n % dp.KBS:] == dp.POISON).all()
        if n >= 48:
            row = inp.bt[b, :n // dp.KBS + 1].tolist()
            assert row != sorted(row) and 0 not in row
        if n >= 1:
            blk = int(inp.bt[b, 0])
            heads = inp.k_cache[:, blk, :, 0].reshape(-1, dp.HD)
            assert torch.unique(heads, dim=0).shape[0] == heads.shape[0]


def test_case_list_covers_the_lengths_and_batches_asked_for():
    ns = {n for c in dp.CASES if c.name.startswith("needle_n") for n in c.ncached}
    assert ns == set(dp.NCACHED)
    assert {c.B for c in dp.CASES} == {1, 2} and {c.L for c in dp.CASES} >= {1, 3}
    assert any(c.B == 2 and -1 in c.ncached for c in dp.CASES)
    assert any(c.B == 2 and min(c.ncached) >= 0 and c.ncached[0] != c.ncached[1] for c in dp.CASES)
    assert {c.G for c in dp.CASES} >= {256, 255, 4}
    assert {c.geo.gq for c in dp.CASES} >= {1, 2, 4, 6, 7, 8}
    assert [dp.case_by_name(n).B for n in dp.BACK_TO_BACK] == [1, 2, 1]


def test_partition_mirror_covers_every_stream_class():
    """Over the case list, each weight stream at each batch size HB runs every row count and piece
    total named in ROW_CLASSES / TOTAL_CLASSES, except those no admissible launch can run
    (dp.unreachable)."""
    seen = set()
    for c in dp.CASES:
        seen |= dp.stream_classes(c.part)
        for s in dp.STREAMS:     # every row has exactly one owner
            n = {"qkv": c.geo.qkvn, "o": c.geo.H, "gu": 2 * c.geo.I, "down": c.geo.H}[s]
            assert sorted(c.part.all_rows(s).tolist()) == list(range(n)), (c.name, s)
    missing = [(s, hb, k) for s in dp.STREAMS for hb in (8, 7, 6) for k in dp.ROW_CLASSES + dp.TOTAL_CLASSES
               if not dp.unreachable(s, hb, k) and (s, hb, k) not in seen]
    assert not missing, missing
    assert not [x for x in seen if dp.unreachable(*x)], "a combination listed as unreachable was reached"
    # GF at four workgroups: 64 O rows and 64 gate / up rows per wave
    p = dp.part(dp.GF, 1, 4)
    assert max(p.counts("o")) == 64 and max(p.counts("gu")) == 64


def test_workspace_mirror_is_consistent():
    for geo in {c.geo for c in dp.CASES}:
        ws = torch.zeros(dp.ws_bytes(geo), dtype=torch.uint8)
        v = dp.ws_views(ws, geo)
        assert v["res"].shape == (2, geo.H) and v["act"].shape == (2, geo.I)
        end = v["act"].data_ptr() + v["act"].numel() * 2 - ws.data_ptr()
        assert end + 1024 == dp.ws_bytes(geo)
        v["err"].fill_(7)
        assert ws.view(torch.int32)[dp.ERR_BYTE // 4] == 7


def test_refusals_of_the_mirror():
    G = dp.Geo
    assert dp.refuses(G(768, 4, 2, 1024), 1) and dp.refuses(G(1024, 4, 2, 768), 1)
    assert dp.refuses(G(512, 2, 1, 512), 1) and dp.refuses(G(2048, 16, 1, 512), 1)
    assert dp.refuses(G(512, 68, 17, 512), 1) and dp.refuses(dp.GA, 3)
    assert dp.refuses(G(8704, 4, 2, 512), 2) and not dp.refuses(G(8704, 4, 2, 512), 1)
    assert dp.refuses(dp.GA, 1, cap=2) and dp.refuses(dp.GA, 1, cap=4) and not dp.refuses(dp.GA, 1, cap=6)


def test_norm_is_exact_whatever_the_last_bit_of_rstd():
    """x = bf16(+-1 rstd g) = +-g for eps <= 1e-5, with rstd one fp32 ulp off either way."""
    g = torch.tensor([1.0, -1.0, 2.0, 4.0])
    for eps in (1e-5, 1e-6, 0.0):
        rstd = torch.rsqrt(torch.tensor(1.0 + eps, dtype=torch.float32))
        for r in (rstd, torch.nextafter(rstd, torch.tensor(0.0)), torch.nextafter(rstd, torch.tensor(2.0))):
            for s in (1.0, -1.0):
                assert torch.equal((s * r * g).to(dp.BF).float(), s * g)


def test_silu_of_the_gate_values_is_exact_in_fp32():
    g = torch.tensor([0.0, 32.0, 64.0])
    assert torch.equal(g / (1.0 + torch.exp(-g)), g)


def _launch_shapes():
    """The first exact case of every (geometry, batch, grid, depth, O mode, MLP mode) in the list."""
    first = {}
    for c in dp.CASES:
        if c.exact:
            first.setdefault((c.geo, c.B, c.cap, c.L, c.o, c.mlp), c)
    return list(first.values())


def _cases_for(m):
    if m.stream is not None or m.name in dp.LAYER_MUTS:
        return _launch_shapes()
    return [c for c in dp.CASES if c.family in ("needle", "count")]


@pytest.mark.parametrize("m", dp.MUTATIONS, ids=dp.mut_id)
def test_mutation_is_rejected(m):
    altered = 0
    for case in _cases_for(m):
        inp, want, emu, clean = _prepared(case.name)
        got, applied = dp.step(inp, "emu", m)
        if not applied or dp.same_outputs(got, clean, case.B):
            continue
        altered += 1
        assert ap.rejects(dp.check, inp, got, want, emu), f"{dp.mut_id(m)} passes at {case.name}"
    assert altered, f"{dp.mut_id(m)} changes nothing at any case"


@pytest.mark.parametrize("stream", ["qkv", "o", "down"])
def test_every_piece_of_a_ledger_row_counts(stream):
    """On the ledger inputs a dropped or doubled piece changes what the test reads at EVERY case
    where the stream's row results are read back as they are: the QKV rows always, the O and down
    rows where they are 'free' integers.  (A 'flip' row of a one-chunk stream whose update is 0 has
    nothing to lose, and a gate / up row shows only through act = g u.)"""
    n = 0
    for m in (dp.Mut("drop_chunk", stream), dp.Mut("double_chunk", stream)):
        for case in _cases_for(m):
            if (stream == "o" and case.o != "free") or (stream == "down" and case.mlp != "free"):
                continue
            inp, want, emu, clean = _prepared(case.name)
            got, applied = dp.step(inp, "emu", m)
            assert applied and not dp.same_outputs(got, clean, case.B), (dp.mut_id(m), case.name)
            n += 1
    assert n >= 20


def _loose(got, want):
    torch.testing.assert_close(got.float(), want.float(), atol=0.1, rtol=0.05)


@pytest.mark.parametrize("m,probe", [(dp.Mut("mask_early"), "needle_n400_last"), (dp.Mut("drop_chunk", "o"), "g0_b1_l1_o")],
                         ids=["lost_token_of_400", "dropped_chunk_of_an_o_row"])
def test_escapes_of_the_loose_comparison(m, probe):
    """What assert_close(atol=0.1, rtol=0.05) on the final hidden state of random weights lets
    through, and the probes do not."""
    if probe == "needle_n400_last":
        case = dp.Case(probe, dp.GA, 1, 1, "needle", (400,), (399,), o="free", mlp="zero", seed=77)
        inp = dp.build(case)
        want, emu = dp.expected(inp)
    else:
        inp, want, emu, _ = _prepared(probe)
    rnd = dp.build_random(dp.Case(inp.case.name + "_random", inp.case.geo, 1, 2, "random", (400,), o="zero", mlp="zero", seed=5))
    clean, _ = dp.step(rnd, "emu")
    broken, applied = dp.step(rnd, "emu", m)
    assert applied and not torch.equal(broken["h_out"], clean["h_out"])
    _loose(broken["h_out"], clean["h_out"])                      # the escape
    got, applied = dp.step(inp, "emu", m)
    assert applied and ap.rejects(dp.check, inp, got, want, emu)  # the probe sees it
