"""csrc/decode_persistent.hip through `ops.decode_persistent` at geometries of a few MB, on inputs
whose answers are known bit for bit (tests/decode_probes.py; what each probe catches is proven on the
CPU by tests/test_decode_probes_cpu.py).

After every launch the error word is 0, ws.qkv / ws.attn / ws.act / ws.res of the last layer, h_out
and both caches (every layer's appended K / V; everything else as before the launch, poison
included) are compared with the fp64 reference: ledger and needle cases with torch.equal, count and
the real-RoPE append with `assert_exact_to_ulp`, random / ramp / rope attention with
`assert_attention_close` (factor 4).  The workspace starts as 0xA5 bytes and is followed by a guard;
h_out is written into the middle of a sentinel frame (ops.decode_persistent's `out`), checked after
every launch, small grids and back-to-back launches included.

Measured on an MI355X (the module prints these again at teardown, see them with -s):
    this module           163 tests, 156 launches, 8.7 s wall (inputs are built on the CPU: about half of it)
    the rest of the suite (every other module of tests/ but this one's CPU sibling): 501 s wall;
                          the CPU sibling (218 tests): about 40 s there
    cases per family      needle 130 (25 geometry / batch / depth, 2 GQA 7, 36 small grids, 67 attention),
                          count 6, random 4, ramp 4, rope 2; plus 4 back-to-back launches, 3 into an output
                          the wrapper allocates, 2 through the entry point without TP arguments, 9 refusals
    count and real-RoPE elements that were the farther bf16 neighbour: 0 of 7808 (limit: one ulp)
    largest random / ramp / rope kernel / emulated ratio: 1.30 (random, B = 2, 600 tokens; limit 4)
Every ledger and needle case was bit-equal, every error word 0, every refusal refused.
"""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected on CPU with -m "not gpu" deselected anyway
    pytest.skip("no GPU", allow_module_level=True)

from ai_agent_kubectl_amd import ops  # noqa: E402
from ai_agent_kubectl_amd.ops import _hip  # noqa: E402
from tests import decode_probes as dp  # noqa: E402

DEV = "cuda"
GUARD = 4096
FRAME, SENTINEL = 1024, -768.0     # elements either side of h_out; no ledger value is beyond +-256
STATE = {"dead": False, "ratio": 0.0, "launches": 0, "families": {}, "ulp": {}, "t0": 0.0}
KEYS = ("wqkv", "wo", "w13", "w2", "ln1", "ln2")


@pytest.fixture(autouse=True, scope="module")
def _lib():
    _hip.require()
    STATE["t0"] = time.time()
    yield
    u = STATE["ulp"]
    print(f"\ndecode probes: {STATE['launches']} launches in {time.time() - STATE['t0']:.1f} s; cases per family "
          f"{STATE['families']}; count / rope elements that are the farther bf16 neighbour: {u.get('farther', 0)} of "
          f"{u.get('n', 0)}; largest ramp / random / rope kernel / emulated ratio {STATE['ratio']:.3f}")


@pytest.fixture(autouse=True)
def _grid(monkeypatch):
    monkeypatch.delenv("KA_PD_GRID", raising=False)


def _workspace(geo):
    n = dp.ws_bytes(geo)
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[:n]


def _ptrs(g):
    return torch.tensor([[l[k].data_ptr() for k in KEYS] for l in g.layers], dtype=torch.int64, device=DEV)


def _launch(monkeypatch, inp, buf=None, framed=True):
    """One launch of a case through ops.decode_persistent -> everything the test reads.  framed: h_out
    goes into the middle of a sentinel frame that must come back whole; else the wrapper allocates it."""
    if STATE["dead"]:
        pytest.skip("an earlier launch of this module set the error word")
    case, geo = inp.case, inp.case.geo
    if case.cap is None:
        monkeypatch.delenv("KA_PD_GRID", raising=False)
    else:
        monkeypatch.setenv("KA_PD_GRID", str(case.cap))
    g = inp.to(DEV)
    if buf is None:
        buf, _ = _workspace(geo)
    ws = buf[:dp.ws_bytes(geo)]
    ptrs = _ptrs(g)
    n = case.B * geo.H
    frame = torch.full((n + 2 * FRAME,), SENTINEL, dtype=dp.BF, device=DEV)
    out = frame[FRAME:FRAME + n].view(case.B, geo.H) if framed else None
    h_out = ops.decode_persistent(g.h0, ptrs, case.L, geo.hq, geo.hkv, geo.I, dp.EPS, dp.SCALE, g.k_cache, g.v_cache,
                                  g.pos, g.slot, g.bt, g.ctx, g.cos_sin, ws, out=out)
    torch.cuda.synchronize()
    STATE["launches"] += 1
    v = dp.ws_views(ws, geo)
    if int(v["err"].item()) != 0:
        STATE["dead"] = True
        pytest.fail(f"{case.name}: the error word is {int(v['err'].item())}: a barrier wait ran out")
    assert (buf[dp.ws_bytes(geo):] == 0xA5).all(), "the guard after the workspace was written"
    if framed:
        assert h_out.data_ptr() == out.data_ptr()
        assert (frame[:FRAME] == SENTINEL).all() and (frame[FRAME + n:] == SENTINEL).all(), \
            f"{case.name}: the frame around h_out was written"
    return dict(qkv=v["qkv"], attn=v["attn"], act=v["act"], res=v["res"], h_out=h_out, k_cache=g.k_cache, v_cache=g.v_cache)


def _run(monkeypatch, case, buf=None, framed=True):
    inp = dp.build(case)
    want, emu = dp.expected(inp)
    got = _launch(monkeypatch, inp, buf, framed)
    r = dp.check(inp, got, want, emu, STATE["ulp"])
    STATE["ratio"] = max(STATE["ratio"], r)
    STATE["families"][case.family] = STATE["families"].get(case.family, 0) + 1
    return inp, got


def test_layout_mirror_matches_the_launcher():
    lib = _hip.require()
    assert int(lib.ka_decode_persistent_err_offset()) == dp.ERR_BYTE
    geos = {c.geo for c in dp.CASES} | {dp.Geo(4096, 32, 8, 14336), dp.Geo(8192, 8, 1, 3584)}
    for geo in geos:
        assert int(lib.ka_decode_persistent_ws(geo.H, geo.hq, geo.hkv, geo.I)) == dp.ws_bytes(geo)
        assert ops.decode_persistent_max_b(geo.H, geo.hq, geo.I, geo.gq) == dp.max_b(geo.H, geo.hq, geo.I, geo.gq)


@pytest.mark.parametrize("case", dp.CASES, ids=lambda c: c.name)
def test_case(monkeypatch, case):
    _run(monkeypatch, case)


def test_back_to_back_on_one_workspace(monkeypatch):
    """B = 1, 2, 1 on the same workspace, different inputs: nothing of a launch (sync words, residual
    rows, the phases' result buffers) reaches the next."""
    geo = dp.case_by_name(dp.BACK_TO_BACK[0]).geo
    buf, _ = _workspace(geo)
    for name in dp.BACK_TO_BACK + dp.BACK_TO_BACK[:1]:
        case = dp.case_by_name(name)
        assert case.geo == geo
        _run(monkeypatch, case, buf)


@pytest.mark.parametrize("name", ["g1_b2_l3_down", "g2_b2_l3_o", "grid4_H1024_hq4_hkv2_I1024_b1"])
def test_wrapper_allocates_h_out_when_given_none(monkeypatch, name):
    _run(monkeypatch, dp.case_by_name(name), framed=False)


def _direct(inp, h_out, ws, B=None, bt_stride=None):
    """The C entry point itself, without the tensor-parallel arguments: -> hipError."""
    case, geo = inp.case, inp.case.geo
    lib = _hip.require()
    p = ops._p
    ptrs = _ptrs(inp)
    rc = lib.ka_decode_persistent(p(h_out), p(inp.h0), p(ptrs), case.L, geo.H, geo.hq, geo.hkv, geo.I, dp.EPS, dp.SCALE,
                                  p(inp.k_cache), p(inp.v_cache), inp.k_cache[0].numel(), p(inp.pos), p(inp.slot),
                                  p(inp.bt), p(inp.ctx), p(inp.cos_sin), p(ws), None, case.B if B is None else B,
                                  inp.bt.stride(0) if bt_stride is None else bt_stride, ops._stream())
    torch.cuda.synchronize()
    return int(rc)


@pytest.mark.parametrize("name", ["g0_b1_l3_down", "g3_b2_pad_l1"])
def test_entry_point_without_tp_arguments(monkeypatch, name):
    """ka_decode_persistent (what a caller without a tensor-parallel group links against), framed."""
    if STATE["dead"]:
        pytest.skip("an earlier launch of this module set the error word")
    case = dp.case_by_name(name)
    inp = dp.build(case)
    want, _ = dp.expected(inp)
    g = inp.to(DEV)
    n, pad = case.B * case.geo.H, FRAME
    frame = torch.full((n + 2 * pad,), SENTINEL, dtype=dp.BF, device=DEV)
    buf, ws = _workspace(case.geo)
    assert _direct(g, frame[pad:pad + n], ws) == 0
    STATE["launches"] += 1
    assert int(dp.ws_views(ws, case.geo)["err"].item()) == 0
    assert (frame[:pad] == SENTINEL).all() and (frame[pad + n:] == SENTINEL).all()
    assert torch.equal(frame[pad:pad + n].view(case.B, -1).double().cpu(), want["h_out"])
    assert (buf[dp.ws_bytes(case.geo):] == 0xA5).all()


def _blank(geo, B):
    """Zero inputs of the right sizes for a launch the host must refuse (were it launched all the
    same, every access would still be in bounds)."""
    z = lambda *s, dt=dp.BF: torch.zeros(*s, dtype=dt, device=DEV)
    case = dp.Case("refused", geo, B, 1, "needle", (0,) * B)
    layer = dict(wqkv=z(geo.qkvn, geo.H), wo=z(geo.H, geo.hq * dp.HD), w13=z(2 * geo.I, geo.H), w2=z(geo.H, geo.I),
                 ln1=z(geo.H), ln2=z(geo.H))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return dp.Inputs(case, z(B, geo.H), [layer], z(1, 4, geo.hkv, dp.KBS, dp.HD), z(1, 4, geo.hkv, dp.HD, dp.KBS),
                     i32([0] * B), i32([16 + b for b in range(B)]), i32([1] * B), i32([[1, 0]] * B), z(4, dp.HD, dt=torch.float32))


REFUSALS = [("H_not_512", dp.Geo(768, 4, 2, 1024), 1, None), ("I_not_512", dp.Geo(1024, 4, 2, 768), 1, None),
            ("hq_2", dp.Geo(512, 2, 1, 512), 1, None), ("gqa_16", dp.Geo(2048, 16, 1, 512), 1, None),
            ("hkv_17", dp.Geo(512, 68, 17, 512), 1, None), ("B_3", dp.GA, 3, None),
            ("B_2_H_8704", dp.Geo(8704, 4, 2, 512), 2, None), ("grid_is_hkv", dp.GA, 1, 2),
            ("more_than_64_rows_per_wave", dp.GA, 1, 4)]


@pytest.mark.parametrize("what,geo,B,cap", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(monkeypatch, what, geo, B, cap):
    """Host checks: an error code, no launch, nothing written."""
    assert dp.refuses(geo, B, cap)
    if cap is not None:
        monkeypatch.setenv("KA_PD_GRID", str(cap))
    inp = _blank(geo, min(B, 3))
    inp.k_cache.fill_(3.0), inp.v_cache.fill_(5.0)
    h_out = torch.full((B, geo.H), SENTINEL, dtype=dp.BF, device=DEV)
    ws = torch.full((dp.ws_bytes(geo),), 0xA5, dtype=torch.uint8, device=DEV)
    assert _direct(inp, h_out, ws, B=B) != 0
    assert (h_out == SENTINEL).all() and (ws == 0xA5).all()
    assert (inp.k_cache == 3.0).all() and (inp.v_cache == 5.0).all()
    if B <= 2:      # and through the wrapper: an exception, not a quiet result
        with pytest.raises(RuntimeError):
            ops.decode_persistent(inp.h0, _ptrs(inp), 1, geo.hq, geo.hkv, geo.I, dp.EPS, dp.SCALE, inp.k_cache,
                                  inp.v_cache, inp.pos, inp.slot, inp.bt, inp.ctx, inp.cos_sin, ws)
        torch.cuda.synchronize()
        assert (ws == 0xA5).all()


def test_the_refused_grids_neighbours_run(monkeypatch):
    """KA_PD_GRID is read on every call: the smallest admissible grids of the refusal cases' geometry."""
    assert not dp.refuses(dp.GA, 1, 6)
    _run(monkeypatch, dp.Case("grid6_after_refusal", dp.GA, 1, 1, "needle", (33,), (32,), o="free", mlp="zero", cap=6, seed=9))
