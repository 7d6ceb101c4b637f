"""Cases of tests/test_logprobs_gpu.py and test_logprobs_cpu.py and their float64 ground truth
(ops/reference.py `token_logprobs`), built once on the CPU and shared.  `python -m tests.logprob_cases`
prints, per case, how far the fp32 form of the definition lies from the float64 truth.

Geometry: the sampler's set (tests/sampling_cases.py) — V = 8 (one vector), 520 (a lane tail), 32776 (one
vector past a whole batch of a workgroup), 128256 (the real row); 1, 3 and 64 rows (64, 16 and 8 slices at
the real row); vocab_offset 0 and 64; with and without mask.  Logits are randn * s, s = 1 and 4 rotating
over the rows, kept to |l| <= 24.  Every case is launched with top_n = 0, 1, 5 and 20 against ONE
reference taken at top_n = 20: the top-n list is a prefix of the top-20 list by definition.

Tolerance of the log-probabilities, LP_TOL = 2e-5 absolute.  A reported value is (l - m) - logf(S):
  * l - m and the final subtraction have magnitude below 64, where an fp32 ulp is 3.8e-6: each rounds
    by at most that (l - m itself is exact: both are bf16 values within 2^6 of each other);
  * logf of S <= V < 2^17 is within a few 1e-6 (|log S| < 12, an ulp there is 9.5e-7, logf is good to
    about an ulp);
  * expf's error (an ulp or two, 1.2e-7 relative per weight) and the truncation to 2^-40 (below
    V * 2^-40 = 1.2e-7 absolute, against S >= 1) move S by less than 1e-6 relative, so log S by that.
The sum stays below 1e-5; 2e-5 leaves a factor of two.  The fp32 reference (this module's __main__)
measured at most 1.0e-6 over all cases.
The mass: out_mass * 2^-40 within MASS_RTOL * S + V * 2^-40 of the float64 sum (expf's relative error
plus one truncation per token).
top ids, the allowed count and the maximum are integers and bf16 values: compared exactly.
"""
import functools

import torch

from ai_agent_kubectl_amd.ops import reference as ref
from tests.sampling_cases import CASES, make_mask

BF = torch.bfloat16
LP_TOL = 2e-5
MASS_RTOL = 1e-6
TOP_NS = (0, 1, 5, 20)
SCALES = (1.0, 4.0)
CLAMP = 24.0


def case_id(c):
    return f"V{c[0]}-R{c[1]}-off{c[2]}-{'mask' if c[3] else 'nomask'}"


def make_logits(R: int, V: int, seed: int, shift: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    s = torch.tensor([SCALES[(r + shift) % len(SCALES)] for r in range(R)])
    return (torch.randn(R, V, generator=g) * s[:, None]).clamp_(-CLAMP, CLAMP).to(BF)


def truth(logits, bits, midx, token, off, top_n=20):
    lp, tid, tlp, mx, cnt, mass = ref.token_logprobs(logits, bits, midx, token, top_n, off, return_probe=True,
                                                     dtype=torch.float64)
    return dict(lp=lp, top_id=tid, top_lp=tlp, max=mx, count=cnt, mass=mass)


@functools.lru_cache(maxsize=None)
def build(case):
    """Inputs (CPU tensors) and the float64 reference (top_n = 20) of one geometry case."""
    V, R, off, masked = case
    no = CASES.index(case)
    logits = make_logits(R, V, 2000 + no, shift=no)
    bits = make_mask(V, off, no) if masked else None
    midx = torch.tensor([(0, -1, 1)[r % 3] for r in range(R)], dtype=torch.int32) if masked else None
    # chosen tokens: the greedy token on even rows (it is top[0]), any id of the slice on odd rows
    greedy, _ = ref.masked_argmax(logits, bits, midx, off)
    g = torch.Generator().manual_seed(3000 + no)
    anyid = torch.randint(0, V, (R,), generator=g, dtype=torch.int32) + off
    token = torch.where(torch.arange(R) % 2 == 0, greedy, anyid).to(torch.int32)
    inp = dict(logits=logits, bits=bits, midx=midx, token=token, off=off)
    return inp, truth(logits, bits, midx, token, off)


@functools.lru_cache(maxsize=None)
def all_equal():
    """V = 32776, masked, every logit 1.0: one key holds the whole row."""
    V, R, off = 32776, 3, 0
    logits = torch.ones(R, V, dtype=BF)
    bits = make_mask(V, off, 97)
    midx = torch.tensor([0, -1, 1], dtype=torch.int32)
    token, _ = ref.masked_argmax(logits, bits, midx, off)
    inp = dict(logits=logits, bits=bits, midx=midx, token=token, off=off)
    return inp, truth(logits, bits, midx, token, off)


@functools.lru_cache(maxsize=None)
def dominated():
    """One token at 24, the rest <= -8 (weights below 2^-40 count as zero): mass == 2^40 exactly."""
    V, R, off = 32776, 3, 64
    logits = make_logits(R, V, 77).clamp_(-CLAMP, -8.0)
    hot = torch.tensor([5, V // 2 + 1, V - 1])
    logits[torch.arange(R), hot] = 24.0
    token = (hot + off).to(torch.int32)
    token[1] = off + 7   # a row whose chosen token is not the dominant one
    inp = dict(logits=logits, bits=None, midx=None, token=token, off=off, hot=hot)
    return inp, truth(logits, None, None, token, off)


def check_close(got_lp: torch.Tensor, want_lp: torch.Tensor, tol: float = LP_TOL) -> float:
    """-inf exactly where the reference has it, |difference| <= tol elsewhere; -> the largest difference."""
    got, want = got_lp.double().flatten(), want_lp.double().flatten()
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and bool((got[inf] < 0).all()), "-inf pattern differs"
    d = (got[~inf] - want[~inf]).abs()
    worst = float(d.max()) if d.numel() else 0.0
    assert worst <= tol, f"max |logprob - float64 reference| = {worst:.3g} > {tol}"
    return worst


def check_mass(got_mass: torch.Tensor, want: dict, V: int) -> None:
    s64 = want["mass"].double() * 2.0 ** -40
    err = (got_mass.double() * 2.0 ** -40 - s64).abs()
    assert bool((err <= MASS_RTOL * s64 + V * 2.0 ** -40).all()), (err, s64)


if __name__ == "__main__":
    import time
    t0 = time.time()
    worst = 0.0
    for case in CASES:
        inp, want = build(case)
        lp, tid, tlp, mx, cnt, mass = ref.token_logprobs(inp["logits"], inp["bits"], inp["midx"], inp["token"], 20,
                                                         inp["off"], return_probe=True)
        assert torch.equal(tid, want["top_id"]) and torch.equal(cnt, want["count"]) and torch.equal(mx, want["max"])
        check_mass(mass, want, case[0])
        e = max(check_close(lp, want["lp"]), check_close(tlp, want["top_lp"]))
        worst = max(worst, e)
        ids0 = want["top_id"][0][want["top_id"][0] >= 0].long() - inp["off"]
        print(f"{case_id(case)}: fp32 reference vs float64: max |d logprob| {e:.3g}; "
              f"distinct values among row 0's top 20: {len(set(inp['logits'][0].float()[ids0].tolist()))}; "
              f"their probability {float(want['top_lp'][0].exp().sum()):.4f}")
    print(f"worst {worst:.3g} (LP_TOL {LP_TOL}), {time.time() - t0:.1f} s")
