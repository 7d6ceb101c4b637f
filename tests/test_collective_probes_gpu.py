"""The probes of tests/collective_probes.py against csrc/allreduce.hip: `world` processes (2, 3, 4) share
the one GPU of the test box, map each other's buffers through hipIpc handles and walk the same case list
tests/test_collective_probes_cpu.py proves sensitive: the plain all-reduce through
OneShotAllReduce.all_reduce and through ka_allreduce_oneshot (trailing workgroups that own nothing,
out != in inside a sentinel frame, a chunk of more than one pass), the all-gather with and without padding
and over several workgroups, the fused all-reduce + residual + RMSNorm at every shape, split count and slab
type with the residual and with residual=None, one sequence that interleaves the three kinds, one captured
graph replayed four times, and the host refusals.

Two groups per process: cap 2^16 (so that n == cap is a case) and cap 2^20 for the fused shapes above 2^16
elements and, at world 2, the 524296-element all-reduce.

A case is run in two steps.  `prepare` builds every input and expectation of the case on the CPU, uploads
the inputs and weights, allocates the sentinel frames and synchronizes.  `fire` then issues the case's
launches and nothing else: no upload, no read-back, no synchronize between them.  The eleven calls of the
sequence therefore sit directly behind one another on the stream (the only kernels in between are the pad
and slice copies of OneShotAllReduce.all_gather at its 4-byte call; the tensors that wrapper allocates are
allocated and freed once in `prepare`, so the caching allocator serves them without a hipMalloc), which is
what hands `ctr` / `done`
from one kernel's last workgroup to the next kernel's first and lets call e + 2 stage into a half while a
peer is as far behind as the protocol allows, at changing workgroup counts.

Between `prepare` and `fire` the ranks exchange one word over gloo ("has anyone failed?"), so the ranks
launch a case within a host round trip of each other whatever the CPU work of `prepare` took on each, and
the kernels' 20 s spin bound never has to absorb host skew.  Every rank issues the identical launch sequence
whatever it finds: mismatches are recorded as (case, what, count, first index, got, want) and reported at
the end.  After every case each rank reads its error word (`check()`) and stops at the first one, or at the
first HIP error; it says so at the next exchange, where its peers, bounded by the spin limit, stop as well,
each with the records it has so far.  The rendezvous is a file store, so no port is picked and freed before
it is used.  The parent opens no GPU, waits for the reports under one deadline (start-up plus the walk plus
one spin bound; 60 s once a rank has reported a failure), names the ranks that did not report, and terminates
whatever is left.  It then asserts, per launch, that the outputs of all ranks are bit-identical.

Measured on the MI355X:

    world  launches/rank  mismatch records  free random   fused output  wall     of which walk (rank 0)
                          (every rank)      |err|/bound   |err|/bound
      2        176              0             0.996         0.996       3.8 s      1.4 s
      3        174              0             0.996         0.996       4.1 s      1.6 s
      4        174              0             0.996         0.996       4.8 s      2.0 s

The exact families (ledger, bounded random, integer probe rows, gather words) have no tolerance: zero
records means torch.equal on every element of every launch, sentinel frames intact, inputs of out != in
launches unchanged, and ctr == launches, done == 0, err == 0 after the refusals, the sequence, the graph
and at the end.  All ranks' digests agree at every launch.  The two ratios are those of the only bounded
comparisons and equal what the torch emulation gives on the CPU.  Wall time is the parent's, from starting
the processes to the last report; pytest's call time is 5.5 / 6.0 / 6.1 s, against 3.2 s for
tests/test_custom_allreduce_gpu.py::test_oneshot_allreduce_two_ranks_one_gpu, which pays the same start-up
for two ranks.

World 8 is not run here.  tests/collective_probes.py and the CPU walk cover it (at most 32 workgroups per
launch, 256 in flight), and this module runs it unchanged if 8 is added to WORLDS, but as a GPU test it
failed once in a run of the whole suite and passed when run again, and the cause was not found: neither in
the kernels' protocol (half reuse, flag monotonicity and the ctr / done hand-over hold at changing workgroup
counts) nor in this harness, whose host skew, port rendezvous and failure path were reworked without
effect.  Eight processes with 32 spinning workgroups each, beside whatever else holds the card, is exactly
the co-residency nobody has measured; until the failing run's message names the case, world 8 on the GPU
is left to a follow-up so that this suite cannot leave up to 256 workgroups spinning on a shared card.
"""
import hashlib
import os
import queue
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_TIMEOUT = 150          # process start-up (imports, IPC set-up of up to 8 ranks) + the walk + one 20 s spin bound
AFTER_FAILURE = 60            # once a rank has reported a failure: one spin bound + one gloo time-out
GLOO_TIMEOUT = 30
DEV = "cuda:0"
WORLDS = (2, 3, 4)            # 8: see the module docstring


class _PeerFailed(RuntimeError):
    pass


class _Walker:
    def __init__(self, rank, world):
        import torch
        import torch.distributed as dist
        from ai_agent_kubectl_amd import ops
        from ai_agent_kubectl_amd.parallel.custom_allreduce import OneShotAllReduce
        from tests import collective_probes as cp
        from tests import elementwise_probes as ep
        self.torch, self.dist, self.ops, self.cp, self.ep = torch, dist, ops, cp, ep
        self.rank, self.world = rank, world
        assert all(OneShotAllReduce.blocks_for(n) == cp.blocks_for(n) for n in (1, 8, 4096, 4104, 12296, 65536, 1 << 20))
        self.groups = {"main": OneShotAllReduce(None, DEV, cap_elems=cp.CAP),
                       "big": OneShotAllReduce(None, DEV, cap_elems=cp.BIG_CAP)}
        self.lib = self.groups["main"].lib
        self.launched = {"main": 0, "big": 0}
        self.records, self.digests = [], []
        self.ratios = {"free": 0.0, "fused": 0.0}
        self.seconds = {}
        self.case = "set-up"

    def report(self):
        return dict(records=self.records, digests=self.digests, ratios=self.ratios, launched=self.launched,
                    seconds=self.seconds, case=self.case)

    def agree(self, failed: bool) -> bool:
        """One word from every rank: True if any rank has failed.  Every rank calls it once per case, between
        `prepare` and `fire`, and once at the end; a rank that fails calls it once more and leaves."""
        t = self.torch.tensor([int(failed)])
        self.dist.all_reduce(t)
        return bool(t.item())

    # ---- prepare: everything a launch needs, on the device; fire: the launch alone -------------------
    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def _rc(self, rc, op):
        if rc != 0:
            raise RuntimeError(f"{op['name']}: launch failed with hipError {rc}")

    def _common(self, ar):
        return (ar._data, ar._flags, ar._ctr, ar._done, ar._err)

    def prepare(self, op, data):
        torch, cp, ep, ops, lib = self.torch, self.cp, self.ep, self.ops, self.lib
        ar = self.groups[op["inst"]]
        rank, world = self.rank, self.world
        pend = dict(op=op, data=data)
        if op["kind"] == "ar":
            src = data["ins"][rank].to(DEV)
            if op["via"] == "wrapper":
                pend["out"] = src
                pend["fire"] = lambda: ar.all_reduce(src)
            else:
                whole, view = ep.framed(1, op["n"], DEV)
                pend.update(out=view[0], whole=whole, in_after=src)
                pend["fire"] = lambda: self._rc(lib.ka_allreduce_oneshot(
                    view.data_ptr(), src.data_ptr(), *self._common(ar), rank, world, op["n"], ar.cap, op["nblocks"],
                    self._stream()), op)
        elif op["kind"] == "ag":
            words = data["ins"][rank]
            if op["via"] == "wrapper":
                t = words.view(op["dtype"])
                t = (t.view(-1, 8) if t.numel() > 8 else t).to(DEV)
                assert t.numel() * t.element_size() == op["nbytes"] and ar.should_gather(t)
                assert ar.blocks_for((op["nbytes"] + 15) // 16 * 8) == op["nblocks"]
                n16 = (op["nbytes"] + 15) // 16 * 8                      # what all_gather will allocate: warm the allocator
                warm = [torch.zeros(n16 * 2, dtype=torch.uint8, device=DEV),
                        torch.empty((world, n16 * 2), dtype=torch.uint8, device=DEV),
                        torch.empty((world, op["nbytes"]), dtype=torch.uint8, device=DEV)]
                del warm

                def fire():
                    out = ar.all_gather(t)
                    assert out.shape == (world,) + tuple(t.shape) and out.dtype == t.dtype
                    pend["out"] = out
                pend["fire"] = fire
            else:
                src = words.view(cp.BF).to(DEV)
                whole, view = ep.framed(world, op["n16"], DEV)
                pend.update(out=view, whole=whole)
                pend["fire"] = lambda: self._rc(lib.ka_allgather_oneshot(
                    view.data_ptr(), src.data_ptr(), *self._common(ar), rank, world, op["n16"], ar.cap, op["nblocks"],
                    self._stream()), op)
        else:
            rows, hidden, split = op["rows"], op["hidden"], op["split"]
            src = data["ins"][rank].to(DEV)
            w = data["w"].to(DEV)
            res = data["res"].to(DEV) if op["with_res"] else None
            whole, view = ep.framed(rows, hidden, DEV)
            pend.update(out=view, whole=whole, res=res)
            if op["via"] == "wrapper":
                assert min(rows, 64) == op["nblocks"]
                t = ops.SplitK(src, split) if split > 1 else src
                assert ar.can_fuse_norm(t)

                def fire():
                    out = ar.all_reduce_rmsnorm(t, w, cp.EPS, res, out=view)
                    assert out.data_ptr() == view.data_ptr()
                pend["fire"] = fire
            else:
                pend["fire"] = lambda: self._rc(lib.ka_allreduce_rmsnorm(
                    view.data_ptr(), src.data_ptr(), res.data_ptr() if res is not None else None, w.data_ptr(), cp.EPS,
                    *self._common(ar), rank, world, rows, hidden, ar.cap, op["nblocks"], split, int(op["slab_bf16"]),
                    self._stream()), op)
        return pend

    def fire(self, pend):
        self.launched[pend["op"]["inst"]] += 1
        pend["fire"]()

    def collect(self, pend):
        """After a synchronize: copy to the CPU, compare, record, digest."""
        torch, cp = self.torch, self.cp
        op, data = pend["op"], pend["data"]
        got = dict(rank=self.rank)
        out = pend["out"].cpu()
        if op["kind"] == "ag":
            out = out.contiguous().view(torch.int16).view(self.world, -1)
        got["out"] = out
        if pend.get("res") is not None:
            got["res"] = pend["res"].cpu()
        if "in_after" in pend:
            got["in_after"] = pend["in_after"].cpu()
        if "whole" in pend:
            whole = pend["whole"]
            edge = torch.cat([whole[:self.ep.PAD], whole[-self.ep.PAD:]])
            got["frame_ok"] = bool((edge == cp.SENT).all())
        rec, ratio = cp.compare(op, data, got)
        self.records += rec
        if ratio is not None:
            key = "free" if op["kind"] == "ar" else "fused"
            self.ratios[key] = max(self.ratios[key], ratio)
        h = hashlib.sha1(got["out"].contiguous().view(torch.int16).numpy().tobytes())
        if got.get("res") is not None:
            h.update(got["res"].contiguous().view(torch.int16).numpy().tobytes())
        self.digests.append((op["name"], h.hexdigest()))

    def check(self):
        """The stop condition: raises at the first error word (HIP errors raise from the synchronize)."""
        for ar in self.groups.values():
            ar.check()

    def state(self, what):
        for inst, ar in self.groups.items():
            ctr, done, err = ar.state.cpu().tolist()[:3]
            if (ctr, done, err) != (self.launched[inst], 0, 0):
                self.records.append((what, f"state of group {inst} (ctr, done, err)", 1, (),
                                     float(ctr), float(self.launched[inst])))
                if done or err:
                    self.records.append((what, f"state of group {inst}: done {done} err {err}", 1, (), float(done), 0.0))

    # ---- the case kinds: prepare_* returns what run_* takes -------------------------------------------
    def prepare_ops(self, ops_):
        pends = [self.prepare(op, self.cp.op_data(op, self.world)) for op in ops_]
        self.torch.cuda.synchronize()
        return pends

    def run_ops(self, pends):
        for p in pends:                                                  # launches only: back to back on the stream
            self.fire(p)
        self.torch.cuda.synchronize()
        for p in pends:
            self.collect(p)

    def prepare_refusals(self):
        torch, cp = self.torch, self.cp
        buf = torch.zeros(1 << 18, dtype=torch.float32, device=DEV)      # large enough for whatever is asked
        out = torch.zeros(1 << 18, dtype=cp.BF, device=DEV)
        w = torch.ones(8200, dtype=cp.BF, device=DEV)
        torch.cuda.synchronize()
        return buf, out, w

    def run_refusals(self, prep):
        cp = self.cp
        buf, out, w = prep
        ar = self.groups["main"]
        for fn, over in cp.refusals():
            a = cp.refusal_args(fn, over, self.world, self.rank)
            if fn == "fused":
                rc = self.lib.ka_allreduce_rmsnorm(out.data_ptr(), buf.data_ptr(), None, w.data_ptr(), cp.EPS,
                                                   *self._common(ar), a["rank"], a["world"], a["rows"], a["hidden"], ar.cap,
                                                   a["nblocks"], a["split"], a["in_bf16"], self._stream())
            else:
                f = self.lib.ka_allreduce_oneshot if fn == "ar" else self.lib.ka_allgather_oneshot
                rc = f(out.data_ptr(), buf.data_ptr(), *self._common(ar), a["rank"], a["world"], a["n"], ar.cap,
                       a["nblocks"], self._stream())
            if rc != cp.INVALID_VALUE:
                self.records.append(("refusals", f"{fn} {over} returned", 1, (), float(rc), float(cp.INVALID_VALUE)))
        self.torch.cuda.synchronize()
        self.state("refusals")                                           # nothing was launched

    def prepare_graph(self, ops_):
        torch, cp, ep = self.torch, self.cp, self.ep
        ar = self.groups["main"]
        a_op, f_op, g_op = ops_[:3]
        x = torch.zeros(a_op["n"], dtype=cp.BF, device=DEV)
        t = torch.zeros(f_op["rows"], f_op["hidden"], dtype=cp.BF, device=DEV)
        r = torch.zeros_like(t)
        w = ep.rms_weight(f_op["hidden"]).to(DEV)
        whole, view = ep.framed(f_op["rows"], f_op["hidden"], DEV)
        src = torch.zeros(g_op["nbytes"] // 4, dtype=g_op["dtype"], device=DEV)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):                          # sequential: no parallel branches
                ar.all_reduce(x)
                ar.all_reduce_rmsnorm(t, w, cp.EPS, r, out=view)
                gout = ar.all_gather(src)
        torch.cuda.synchronize()
        self.state("graph capture")                                      # capture launches nothing
        datas = [cp.op_data(o, self.world) for o in ops_]
        return dict(g=g, x=x, t=t, r=r, w=w, whole=whole, view=view, src=src, gout=gout, datas=datas, stream=s)

    def run_graph(self, ops_, p):
        torch = self.torch
        for rep in range(self.cp.GRAPH_REPLAYS):
            trio = ops_[3 * rep:3 * rep + 3]
            datas = p["datas"][3 * rep:3 * rep + 3]
            p["x"].copy_(datas[0]["ins"][self.rank])
            p["t"].copy_(datas[1]["ins"][self.rank])
            p["r"].copy_(datas[1]["res"])
            p["src"].copy_(datas[2]["ins"][self.rank].view(p["src"].dtype))
            torch.cuda.synchronize()
            p["g"].replay()
            torch.cuda.synchronize()
            for o in trio:
                self.launched[o["inst"]] += 1
            self.collect(dict(op=trio[0], data=datas[0], out=p["x"]))
            self.collect(dict(op=trio[1], data=datas[1], out=p["view"], whole=p["whole"], res=p["r"]))
            self.collect(dict(op=trio[2], data=datas[2], out=p["gout"]))
        self.state("graph")

    def _walk(self):
        t0 = time.time()
        for case in self.cp.cases(self.world):
            t1 = time.time()
            self.case = case["name"]
            kind = case["kind"]
            if kind == "refusals":
                prep = self.prepare_refusals()
            elif kind == "graph":
                prep = self.prepare_graph(case["ops"])
            else:
                prep = self.prepare_ops(case["ops"])
            if self.agree(False):
                raise _PeerFailed(f"stopped before the launches of case {self.case}: a peer reported a failure")
            if kind == "refusals":
                self.run_refusals(prep)
            elif kind == "graph":
                self.run_graph(case["ops"], prep)
            else:
                self.run_ops(prep)
                if kind == "sequence":
                    self.state("sequence")
            self.check()
            self.seconds[kind] = self.seconds.get(kind, 0.0) + time.time() - t1
        self.case = "end"
        self.state("end")
        self.seconds["walk"] = time.time() - t0
        if self.agree(False):
            raise _PeerFailed("a peer reported a failure in the last case")

    def walk(self):
        try:
            self._walk()
        except _PeerFailed:
            raise
        except Exception:
            try:
                self.agree(True)                   # tell the peers at the exchange they are heading for
            except Exception:                      # pragma: no cover - the peers are gone
                pass
            raise
        return self.report()


def _worker(rank, world, store_path, q):
    wk = None
    try:
        t0 = time.time()
        sys.path.insert(0, ROOT)
        import datetime
        import torch
        import torch.distributed as dist
        torch.set_num_threads(2)
        store = dist.FileStore(store_path, world)
        dist.init_process_group("gloo", store=store, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=GLOO_TIMEOUT))
        torch.cuda.set_device(0)
        wk = _Walker(rank, world)
        setup = time.time() - t0
        report = wk.walk()
        report["seconds"]["setup"] = setup
        q.put((rank, report, None))
    except Exception:  # pragma: no cover - reported to the parent, with what the rank had recorded
        import traceback
        q.put((rank, wk.report() if wk is not None else None, traceback.format_exc()))
        return
    for ar in wk.groups.values():                  # every rank is past its last kernel: the final exchange said so
        ar.close()


def _run(world, store_path):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, store_path, q)) for r in range(world)]
    t0 = time.time()
    for p in procs:
        p.start()
    res = {}
    deadline = t0 + REPORT_TIMEOUT
    try:
        while len(res) < world:
            try:
                r, rep, tb = q.get(timeout=max(0.1, deadline - time.time()))
            except queue.Empty:
                missing = sorted(set(range(world)) - set(res))
                tbs = "\n".join(f"rank {r} (in case {rep and rep['case']}, records {rep and rep['records'][:5]}):\n{tb}"
                                for r, (rep, tb) in sorted(res.items()) if tb)
                pytest.fail(f"world {world}: ranks {missing} did not report in time\n{tbs}")
            res[r] = (rep, tb)
            if tb:
                deadline = min(deadline, time.time() + AFTER_FAILURE)
    finally:
        ok = len(res) == world and not any(tb for _, tb in res.values())
        end = time.time() + (30 if ok else 3)                          # one deadline for all, then no survivors
        for p in procs:
            p.join(timeout=max(0.0, end - time.time()))
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=5)
            if p.is_alive():
                p.kill()
    return res, time.time() - t0


@pytest.mark.parametrize("world", WORLDS)
def test_collective_probes(world, tmp_path):
    from tests import collective_probes as cp
    res, wall = _run(world, str(tmp_path / "rendezvous"))
    tbs = [f"rank {r}, in case {rep and rep['case']}, {rep and len(rep['records'])} mismatch records so far "
           f"(first five: {rep and rep['records'][:5]}):\n{tb}" for r, (rep, tb) in sorted(res.items()) if tb]
    assert not tbs, "\n".join(tbs)
    reps = {r: rep for r, (rep, _) in res.items()}
    nrec = {r: len(rep["records"]) for r, rep in sorted(reps.items())}
    free = max(rep["ratios"]["free"] for rep in reps.values())
    fused = max(rep["ratios"]["fused"] for rep in reps.values())
    sec = reps[0]["seconds"]
    print(f"\nworld {world}: {cp.launches(world) + cp.launches(world, 'big')} launches per rank, mismatch records per rank "
          f"{nrec}; largest |got - want| / bound: free random {free:.3f}, fused output {fused:.3f}; wall {wall:.1f} s "
          f"(rank 0: " + ", ".join(f"{k} {v:.2f}" for k, v in sec.items()) + ")")
    for r, rep in sorted(reps.items()):
        assert not rep["records"], f"rank {r}: {len(rep['records'])} mismatches, first ten: {rep['records'][:10]}"
        assert rep["launched"] == {"main": cp.launches(world), "big": cp.launches(world, "big")}
    names = [n for n, _ in reps[0]["digests"]]
    assert len(names) == cp.launches(world) + cp.launches(world, "big")
    for r, rep in sorted(reps.items()):                   # every rank ends with the same bits
        diff = [n for (n, d), (_, d0) in zip(rep["digests"], reps[0]["digests"]) if d != d0]
        assert [n for n, _ in rep["digests"]] == names and not diff, f"rank {r} differs from rank 0 in {diff[:10]}"
    assert free <= 1 and fused <= 1
