"""The multi-GPU path on the hardware that is there (one MI355X): the collective of the design under RCCL with a single rank, the
benchmark's sharded run launched the way the driver launches it, and concurrent provers inside one process.  World size 2 runs on
CPU under gloo (tests/test_distributed_cpu.py)."""
import json
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_gather_roots_over_rccl_single_rank():
    """shard.gather_roots with device tensors through the nccl (= RCCL) backend, world size 1, in a subprocess of its own"""
    code = r'''
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from stark_brainfuck_amd import shard
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
roots = {c: bytes([c + 1]) * 64 for c in range(5)}
# world size 1 short-circuits inside gather_roots; force the collective path through the private helper
out = shard.gather_roots(roots, 5, 1, 0, device=torch.device("cuda", 0), force_collective=True)
assert out == [roots[c] for c in range(5)], out
dist.barrier(); dist.destroy_process_group()
print("ok")
''' % ROOT
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout + res.stderr


def test_all_gather_rows_over_rccl_single_rank():
    """shard.all_gather_rows on the library's own device memory wrapped as torch tensors (no copy), nccl (= RCCL) backend, world size 1:
    the device path a cooperative proof takes with the combination codeword"""
    code = r'''
import os, sys
sys.path.insert(0, %r)
import numpy as np
import torch, torch.distributed as dist
from stark_brainfuck_amd import shard
from stark_brainfuck_amd.device import DeviceBuffer
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
n, stride = 1 << 12, (1 << 12) + 8
data = np.arange(3 * stride, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
buf = DeviceBuffer.from_numpy(data)
view = torch.as_tensor(shard._DeviceWords(buf.ptr + 8 * stride, n), device=torch.device("cuda", 0))
assert view.data_ptr() == buf.ptr + 8 * stride                       # a window, not a copy
assert (view.cpu().numpy().view(np.uint64) == data[stride:stride + n]).all()
shard.all_gather_rows(buf.ptr, n, 3, stride, 1, 0, device=torch.device("cuda", 0), force_collective=True)
assert (buf.to_numpy() == data).all()                                # one rank: the gather is the identity, through the collective
dist.barrier(); dist.destroy_process_group()
print("ok")
''' % ROOT
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout + res.stderr


@pytest.mark.parametrize("scaling", ["strong", "weak"])
def test_bench_under_torchrun_single_rank(scaling):
    """bench.py launched exactly as the driver launches N > 1 (torch.distributed.run, RCCL process group), with the one rank this
    box has: sharding through shard.assign_columns, the all-gather of the roots, one JSON line with the contract's keys"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--scaling", scaling, "--total-columns", "4", "--columns", "2", "--log-n", "20", "--full", "--no-fri", "--no-cpu", "--spinup-ms", "0"]
    res = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in line, key
    assert line["scaling"] == scaling and line["n_gpus"] == 1 and line["steps"] == 3
    assert line["config"]["total_columns"] == (4 if scaling == "strong" else 2)
    assert line["roots_sha256"] and len(line["roots_sha256"]) == 64
    assert line["value"] > 1e9


def test_plain_bench_times_the_headline_and_dumps_the_last_step(oracle, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`, no --full: the line carries the headline keys and none of the other
    legs, and the dumped sample (here every element: two 2^12 columns are under the 2^20 budget) is the oracle's forward transform of
    the bench's inputs -- the limbs exactly, the rounded float64 to the last place"""
    n, cols = 1 << 12, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--log-n", "12",
           "--total-columns", str(cols), "--spinup-ms", "0", "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 4 and line["ms_per_step"] > 0
    for key in ("cpu_baseline", "sustained", "fri_prove", "stark_prove", "single_column_2p24", "merkle_tree_2p24"):
        assert key not in line, key
    assert line["guard"] is None and line["roots_sha256"] is None and line["ms_per_step_direct_route"] is None
    import bench                    # (ROOT is on sys.path: conftest)
    w = oracle.primitive_nth_root(n)
    want = np.stack([oracle.ntt(w, bench.felt_array(bench.SEED + (c << 32), 0, n)) for c in range(cols)])
    idx = np.load(tmp_path / "ntt_output_index.npy")
    limbs = np.load(tmp_path / "ntt_output_limbs16.npy")
    vals = np.load(tmp_path / "ntt_output.npy")
    assert idx.shape == (cols, n) and (idx == np.arange(n)).all()
    assert limbs.dtype == np.float32 and vals.dtype == np.float64 and limbs.shape == (cols, n, 4)
    got = sum(limbs[..., i].astype(np.uint64) << np.uint64(16 * i) for i in range(4))
    assert (got == want).all()
    assert (vals == want.astype(np.float64)).all()


def test_concurrent_provers_in_one_process(oracle):
    """two threads, each with its own stream, run Fri.prove on different codewords at the same time: the transcripts must be the
    oracle's (the gather staging is leased per call, the scratch areas are keyed by (device, stream))"""
    import ctypes
    from stark_brainfuck_amd import _lib
    from stark_brainfuck_amd.device import DeviceBuffer
    lib = _lib.load()
    N, d, t, expansion = 1 << 12, 1 << 10, 4, 4
    log_n = 12
    omega = oracle.primitive_nth_root(N)
    results, errors = {}, []

    def worker(k):
        try:
            stream = ctypes.c_void_p()
            _lib.check(lib.bfs_stream_create(ctypes.byref(stream)))
            coeffs = oracle.felt_array(0x5EED + 77 * k, 0, 3 * d).reshape(d, 3).T.copy()
            soa = oracle.xevaluate_soa(coeffs, 7, omega, N)
            cw = DeviceBuffer.from_numpy(np.ascontiguousarray(soa).reshape(-1))
            for rep in range(6):
                ps = lib.bfs_ps_new()
                out = (ctypes.c_uint64 * t)()
                _lib.check(lib.bfs_fri_prove(ps, cw.ptr, N, log_n, 7, omega, expansion, t, out, stream))
                size = ctypes.c_size_t()
                _lib.check(lib.bfs_ps_serialize(ps, 1 << 62, None, 0, ctypes.byref(size)))
                buf = ctypes.create_string_buffer(size.value)
                _lib.check(lib.bfs_ps_serialize(ps, 1 << 62, buf, size.value, ctypes.byref(size)))
                lib.bfs_ps_free(ps)
                results.setdefault(k, []).append(([int(v) for v in out], buf.raw[:size.value]))
            results[(k, "soa")] = soa
            _lib.check(lib.bfs_stream_synchronize(stream))
            _lib.check(lib.bfs_stream_destroy(stream))
        except Exception as e:              # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(3):
        ref = oracle.fri_prove(results[(k, "soa")], 7, omega, expansion, t)
        for idx, raw in results[k]:
            assert idx == ref["indices"]
            assert raw == ref["proof_stream"].serialize()


def _gpu_sharded_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from stark_brainfuck_amd import shard
    from stark_brainfuck_amd.device import DeviceBuffer
    from stark_brainfuck_amd.salted_merkle import ZippedSaltedMerkle
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # both ranks compute on the one GPU; the exchange runs over gloo
    P = (1 << 64) - (1 << 32) + 1
    n = 1 << 12
    rng = np.random.default_rng(99)
    planes = [3, 1, 1, 3, 1, 1, 3]
    columns = [rng.integers(0, P, (p, n), dtype=np.uint64) for p in planes]
    columns[3][1:, ::3] = 0                                            # extension elements with fewer stored coefficients
    columns[1][0, ::5] = 7
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    mine = shard.assign_columns(len(planes), world, rank)
    local = {c: torch.from_numpy(columns[c].view(np.int64).copy()) for c in mine}
    tree = shard.ShardedZippedMerkle(local, planes, n, world, rank, shard.gpu_subtree_builder([p == 3 for p in planes]), salts=salts)
    opened = {i: tree.open(i) for i in sorted({0, n // world - 1, (n // world) % n, n - 1})}
    whole = None
    if rank == 0:
        bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(c).reshape(-1)) for c in columns]
        full = ZippedSaltedMerkle([(b.ptr, p == 3, 0) for b, p in zip(bufs, planes)], n, lambda i: None, salts=salts)
        whole = (full.root().hex(), {i: (full.open(i)[0].hex(), [x.hex() for x in full.open(i)[1]]) for i in opened})
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, tree.root().hex(), {i: (s.hex(), [x.hex() for x in p]) for i, (s, p) in opened.items()}, whole))


@pytest.mark.parametrize("world", [1, 2, 4])
def test_row_sharded_commitment_on_the_gpu(world):
    """shard.ShardedZippedMerkle with the zipped-row leaf kernel hashing each rank's row range: root and authentication paths equal
    those of the one tree over all rows (bfs_merkle_build_rows), for 1, 2 and 4 ranks sharing this GPU"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gpu_sharded_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    for _ in procs:
        for attempt in range(90):                      # a worker that died leaves nothing in the queue: do not wait for it
            try:
                got.append(q.get(timeout=2))
                break
            except Exception:
                assert all(p.is_alive() or p.exitcode == 0 for p in procs), "a worker failed: %r" % [p.exitcode for p in procs]
        else:
            raise AssertionError("timed out")
    got.sort(key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    root, paths = got[0][3]
    for rank, r, opened, _ in got:
        assert r == root, rank
        assert opened == paths, rank


def _coop_worker(rank, world, port, name, q):
    import hashlib
    import json
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from stark_brainfuck_amd import brainfuck_stark, salted_merkle, shard, table
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.vm import VirtualMachine
    from test_gpu_stark import Stream
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "stark_%s.json" % name)))
    program = VirtualMachine.compile(g["program"])
    running_time, inputs, outputs = VirtualMachine.run(program, input_data=list(g["input"]))
    matrices = VirtualMachine.simulate(program, input_data=list(inputs))
    # (1) the reference's byte stream as os.urandom on every rank: the cooperative proof must be the reference's proof
    stream = Stream(name.encode())
    for mod in (brainfuck_stark, salted_merkle, table):
        mod.urandom = stream
    stark = BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs).cooperate(world, rank)
    proof = stark.prove(program, *matrices)
    golden_ok = hashlib.sha256(proof).hexdigest() == g["proof_sha256"] and stream.pos == g["urandom_bytes"]
    # (2) production randomness: one seed from rank 0, shared
    import os as _os
    for mod in (brainfuck_stark, salted_merkle, table):
        mod.urandom = _os.urandom
    with shard.shared_randomness(world, rank):
        fresh = BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs).cooperate(world, rank).prove(program, *matrices)
    assert brainfuck_stark.urandom is _os.urandom
    verified = BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs).verify(fresh)
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, golden_ok, hashlib.sha256(fresh).hexdigest(), bool(verified), len(proof)))


@pytest.mark.parametrize("name,world", [("loop", 2), ("two_io", 4)])
def test_cooperative_proof_is_the_reference_proof(name, world):
    """BrainfuckStark.cooperate(): `world` provers (sharing this GPU, exchanging over gloo) hash disjoint row ranges of the zipped
    commitments and exchange subtree roots and opened paths; with the reference's randomness every rank writes the reference's
    proof (tests/golden), with shared fresh randomness all ranks write the same proof and verify() accepts it"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_coop_worker, args=(r, world, port, name, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    for _ in procs:
        for attempt in range(150):
            try:
                got.append(q.get(timeout=2))
                break
            except Exception:
                assert all(p.is_alive() or p.exitcode == 0 for p in procs), "a worker failed: %r" % [p.exitcode for p in procs]
        else:
            raise AssertionError("timed out")
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _, _, _ in got), "a rank's proof differs from the reference's"
    assert len({h for _, _, h, _, _ in got}) == 1, "the ranks wrote different proofs"
    assert all(v for _, _, _, v, _ in got)


def test_bench_with_two_ranks_on_one_gpu():
    """the N > 1 code path of bench.py -- columns split by shard.assign_columns, max over ranks, replicas' all-gathers, the all-gather of
    the roots, and the cooperative proof -- with two ranks that share this GPU and exchange over gloo (BFS_BENCH_BACKEND / _DEVICE)"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--total-columns", "4", "--log-n", "20", "--full", "--no-cpu", "--spinup-ms", "0", "--cooperative"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BFS_BENCH_BACKEND="gloo", BFS_BENCH_DEVICE="0")
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["columns_per_gpu"] == [2, 2]
    assert len(line["fri_prove"]["replicas"]["per_gpu_ms"]) == 2 and len(line["stark_prove"]["replicas"]["per_gpu_ms"]) == 2
    assert line["stark_prove"]["verified"] is True
    assert line["stark_prove_cooperative"]["ranks"] == 2 and line["stark_prove_cooperative"]["verified"] is True
    assert line["roots_sha256"]


def test_bench_with_eight_ranks_on_one_gpu():
    """the rank count the driver's scaling run uses (`bench.py --gpus 8`): eight ranks share this box's one GPU and exchange over gloo.
    One column per rank (`columns_per_gpu [1] * 8`, shard.assign_columns), every replica leg all-gathered over eight ranks, the roots
    of all eight columns gathered, and the cooperative proof of world size 8 (row ranges of 1/8 of the domain, eight subtree roots)
    equal to what verify() accepts.  No scaling number comes out of this -- it exercises the code path at the driver's world size."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--total-columns", "8", "--log-n", "20", "--full", "--no-cpu", "--spinup-ms", "0", "--cooperative", "--no-single", "--no-concurrent"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BFS_BENCH_BACKEND="gloo", BFS_BENCH_DEVICE="0")
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=2400, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["scaling"] == "strong" and line["config"]["columns_per_gpu"] == [1] * 8
    assert line["rccl_ranks_seen"] == 8 and len(line["rank_devices"]) == 8
    assert len(line["fri_prove"]["replicas"]["per_gpu_ms"]) == 8 and len(line["stark_prove"]["replicas"]["per_gpu_ms"]) == 8
    assert line["stark_prove"]["verified"] is True
    assert line["stark_prove_cooperative"]["ranks"] == 8 and line["stark_prove_cooperative"]["verified"] is True
    assert line["guard"]["columns_round_tripped"] == 1 and line["roots_sha256"]


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_bench_fails_loudly_when_the_communicator_does_not_come_up(backend):
    """round-5 verdict, next #8: a rank whose peers never arrive must end with a non-zero status and a line on stderr that names the rank
    and the stage it was stuck in, within the limit (BFS_BENCH_COMM_TIMEOUT_S, 120 s by default; 8 s here) -- not hang the scaling run.
    Rank 0 of a two-rank job is started alone: the rendezvous can never complete."""
    import time
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BFS_BENCH_BACKEND=backend, BFS_BENCH_DEVICE="0", BFS_BENCH_COMM_TIMEOUT_S="8",
               RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    env.pop("TORCHELASTIC_RUN_ID", None)
    t0 = time.time()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--log-n", "16", "--no-cpu",
                          "--no-fri", "--no-stark"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    took = time.time() - t0
    assert res.returncode != 0, res.stdout[-1000:]
    assert took < 120, took
    assert "did not come up within" in res.stderr or "imeout" in res.stderr, res.stderr[-2000:]
    assert not [l for l in res.stdout.splitlines() if l.startswith("{")], "no JSON line may be printed by a job that did not run"


def test_plain_bench_command_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it (what a driver that reuses its N = 1 command line runs): bench.py starts
    the two ranks itself under torch.distributed.run and rank 0's JSON line arrives on the caller's stdout; the cooperative proof runs as
    bench.guarded_cooperative's separate job.  Two ranks share this
    box's one GPU and exchange over gloo (test hooks BFS_BENCH_BACKEND / BFS_BENCH_DEVICE)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--total-columns", "4",
           "--log-n", "20", "--full", "--no-cpu", "--spinup-ms", "0"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", BFS_BENCH_BACKEND="gloo", BFS_BENCH_DEVICE="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["rccl_ranks_seen"] == 2 and len(line["rank_devices"]) == 2
    assert line["config"]["columns_per_gpu"] == [2, 2]
    assert line["guard"]["columns_round_tripped"] == 2 and line["roots_sha256"]
    # ... and, with no flag asking for it, the cooperative proof as a separate time-limited job started by rank 0 afterwards
    coop = line["stark_prove_cooperative"]
    assert coop.get("separate_job") is True and coop.get("ranks") == 2 and coop.get("verified") is True, coop


def _rccl_worker(rank, world, port, q):
    """one rank per GPU over RCCL: every collective of shard.py on CUDA buffers, then a cooperative proof"""
    import hashlib
    import json
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from stark_brainfuck_amd import _lib, brainfuck_stark, salted_merkle, shard, table
    from stark_brainfuck_amd.brainfuck_stark import BrainfuckStark
    from stark_brainfuck_amd.device import DeviceBuffer
    from stark_brainfuck_amd.salted_merkle import ZippedSaltedMerkle
    from stark_brainfuck_amd.vm import VirtualMachine
    from test_gpu_stark import Stream
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(rank)
    _lib.check(_lib.load().bfs_set_device(rank))
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    props = torch.cuda.get_device_properties(rank)
    out = {"rank": rank, "rccl_ranks_seen": dist.get_world_size(), "device": rank, "name": props.name,
           "pci_bus_id": getattr(props, "pci_bus_id", None), "uuid": str(getattr(props, "uuid", "")) or None}
    # (1) gather_roots: the all-gather of 64-byte roots (5 columns over `world` ranks: uneven)
    roots = {c: bytes([c + 1]) * 64 for c in shard.assign_columns(5, world, rank)}
    out["roots_ok"] = shard.gather_roots(roots, 5, world, rank, device=dev) == [bytes([c + 1]) * 64 for c in range(5)]
    # (2) exchange_rows (all_to_all_single on CUDA tensors) inside ShardedZippedMerkle, against the one tree over all rows
    P = (1 << 64) - (1 << 32) + 1
    n = 1 << 12
    rng = np.random.default_rng(99)
    planes = [3, 1, 1, 3, 1, 1, 3]
    columns = [rng.integers(0, P, (p, n), dtype=np.uint64) for p in planes]
    columns[3][1:, ::3] = 0
    salts = rng.integers(0, 256, 24 * n, dtype=np.uint8).tobytes()
    local = {c: torch.from_numpy(columns[c].view(np.int64).copy()).to(dev) for c in shard.assign_columns(len(planes), world, rank)}
    tree = shard.ShardedZippedMerkle(local, planes, n, world, rank, shard.gpu_subtree_builder([p == 3 for p in planes]), salts=salts, device=dev)
    opened = {i: tree.open(i) for i in sorted({0, n // world - 1, (n // world) % n, n - 1})}
    bufs = [DeviceBuffer.from_numpy(np.ascontiguousarray(c).reshape(-1)) for c in columns]
    full = ZippedSaltedMerkle([(b.ptr, p == 3, 0) for b, p in zip(bufs, planes)], n, lambda i: None, salts=salts)
    out["zipped_ok"] = tree.root() == full.root() and all(
        (s, p) == (full.open(i)[0], list(full.open(i)[1])) for i, (s, p) in opened.items())
    # (3) all_gather_rows on the library's own device memory: every rank fills its rows of 3 planes
    stride = n + 8
    data = (np.arange(3 * stride, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) % np.uint64(P)
    first, m = shard.row_range(n, world, rank)
    part = np.zeros_like(data)
    for pl in range(3):
        part[pl * stride + first:pl * stride + first + m] = data[pl * stride + first:pl * stride + first + m]
    buf = DeviceBuffer.from_numpy(part)
    shard.all_gather_rows(buf.ptr, n, 3, stride, world, rank, device=dev)
    got = buf.to_numpy()
    out["rows_ok"] = all((got[pl * stride:pl * stride + n] == data[pl * stride:pl * stride + n]).all() for pl in range(3))
    # (4) a cooperative proof with the reference's byte stream on every rank: every rank writes the reference's proof
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "stark_loop.json")))
    program = VirtualMachine.compile(g["program"])
    running_time, inputs, outputs = VirtualMachine.run(program, input_data=list(g["input"]))
    matrices = VirtualMachine.simulate(program, input_data=list(inputs))
    stream = Stream(b"loop")
    for mod in (brainfuck_stark, salted_merkle, table):
        mod.urandom = stream
    proof = BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs).cooperate(world, rank, device=dev).prove(program, *matrices)
    out["proof_ok"] = hashlib.sha256(proof).hexdigest() == g["proof_sha256"]
    for mod in (brainfuck_stark, salted_merkle, table):
        mod.urandom = os.urandom
    with shard.shared_randomness(world, rank):
        fresh = BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs).cooperate(world, rank, device=dev).prove(program, *matrices)
    out["fresh_sha"] = hashlib.sha256(fresh).hexdigest()
    out["fresh_verified"] = bool(BrainfuckStark(running_time, len(matrices[1]), program, inputs, outputs).verify(fresh))
    dist.barrier()
    dist.destroy_process_group()
    q.put(out)


def test_rccl_worker_with_the_one_rank_this_box_has():
    """the worker of the multi-GPU test below, with world size 1 under RCCL: the same code path end to end on a one-GPU box (the
    collectives degenerate, the comparisons do not)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = ctx.Process(target=_rccl_worker, args=(0, 1, _free_port(), q))
    p.start()
    o = None
    for attempt in range(300):
        try:
            o = q.get(timeout=2)
            break
        except Exception:
            assert p.is_alive() or p.exitcode == 0, "the worker failed: %r" % p.exitcode
    p.join(60)
    assert p.exitcode == 0 and o is not None
    assert o["roots_ok"] and o["zipped_ok"] and o["rows_ok"] and o["proof_ok"] and o["fresh_verified"], o


def test_collectives_and_cooperative_proof_over_rccl_one_rank_per_gpu():
    """needs >= 2 GPUs (skipped on a one-GPU box): gather_roots, exchange_rows (inside ShardedZippedMerkle), all_gather_rows and a
    cooperative proof with ONE RANK PER GPU over RCCL, each compared with what a single GPU computes -- the first multi-GPU box to
    run this suite exercises every collective of the design under pytest, not only inside bench.py (round-3 verdict #5b;
    the split under test: /root/reference/code/brainfuck_stark.py:178-180)"""
    import torch
    count = torch.cuda.device_count()
    if count < 2:
        pytest.skip("one GPU: the RCCL collectives between GPUs cannot run here (world size 1 and gloo variants above do)")
    world = 4 if count >= 4 else 2
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [ctx.Process(target=_rccl_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    try:
        for _ in procs:
            for attempt in range(300):
                try:
                    got.append(q.get(timeout=2))
                    break
                except Exception:
                    assert all(p.is_alive() or p.exitcode == 0 for p in procs), "a worker failed: %r" % [p.exitcode for p in procs]
            else:
                raise AssertionError("timed out")
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:                 # a rank stuck in a collective must not outlive the test
            if p.is_alive():
                p.kill()
    # what the first multi-GPU box should put on record (pytest -s / the captured output of a failure): who was in the job
    print("rccl_ranks_seen", sorted({o["rccl_ranks_seen"] for o in got}), "ranks", world, "devices",
          [(o["rank"], o["device"], o.get("pci_bus_id"), o.get("uuid")) for o in sorted(got, key=lambda o: o["rank"])])
    assert all(o["rccl_ranks_seen"] == world for o in got)
    ids = [o.get("uuid") or (o["device"], o.get("pci_bus_id")) for o in got]
    assert len(set(map(str, ids))) == world, "ranks must sit on distinct GPUs: %r" % ids
    for o in got:
        assert o["roots_ok"] and o["zipped_ok"] and o["rows_ok"] and o["proof_ok"] and o["fresh_verified"], o
    assert len({o["fresh_sha"] for o in got}) == 1
    # bench.py as the driver runs it, at N = 1 and at N = world, on this box: the N-rank line must name `world` ranks and distinct
    # devices, and its whole-job value must agree with N x the one-GPU value (strong scaling over 8 columns: >= 0.6 x linear -- the
    # step is HBM / issue bound per GPU and shares nothing but the 64-byte roots)
    import json
    import subprocess
    import sys
    lines = {}
    for gpus in (1, world):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "10", "--warmup", "2", "--no-fri", "--no-stark",
                              "--no-cpu", "--no-single", "--no-concurrent", "--no-cooperative"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        lines[gpus] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
        print("bench --gpus %d: value %.4g %s, ms_per_step %.4f, rccl_ranks_seen %s" % (gpus, lines[gpus]["value"], lines[gpus]["unit"],
                                                                                          lines[gpus]["ms_per_step"], lines[gpus].get("rccl_ranks_seen")))
    assert lines[world]["n_gpus"] == world and lines[world].get("rccl_ranks_seen") == world
    assert lines[world]["value"] >= 0.6 * world * lines[1]["value"], (lines[1]["value"], lines[world]["value"])
