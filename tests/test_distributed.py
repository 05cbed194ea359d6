"""The N > 1 path on CPU: world_size-2 gloo process group, one emulated 'GPU' per rank,
contiguous shards, host-side gather -- result must equal the single-process run."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, total, out_path):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from atropos_amd import _lib, shard, synth
    from atropos_amd.align import Aligner
    from tests.emu.backend import EmuBackend
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _lib.set_backend(EmuBackend(), _test_double=True)
    w = synth.workload("C2", 0, total)
    al = Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
    local, gathered = shard.sharded_locate(al, w["reads"])
    lo, hi = shard.shard_range(total, rank, world)
    assert len(local) == hi - lo
    if rank == 0:
        torch.save(gathered, out_path)
    else:
        assert gathered is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,total", [(2, 1000), (2, 1001), (3, 130)])
def test_sharded_locate_matches_single_process(tmp_path, emu_backend, world, total):
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    out_path = str(tmp_path / "gathered.pt")
    mp.spawn(_worker, args=(world, _free_port(), total, out_path), nprocs=world, join=True)
    gathered = torch.load(out_path)
    w = synth.workload("C2", 0, total)
    al = Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
    single = al.locate_batch(w["reads"]).records
    assert gathered.shape == single.shape
    assert torch.equal(gathered, single)


def test_shard_range_partition():
    from atropos_amd.shard import shard_range
    for total in (0, 1, 7, 64, 1000, 1001):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert all(lo <= hi for lo, hi in spans)


def _trim_worker(rank, world, port, path_in, path_out, args):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from atropos_amd import _lib, shard
    from atropos_amd.trim import pipeline_from_args
    from tests.emu.backend import EmuBackend
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _lib.set_backend(EmuBackend(), _test_double=True)
    counts = shard.sharded_trim_file(pipeline_from_args(args), path_in, path_out, chunk_bytes=40000)
    total = torch.tensor([sum(counts.values())], dtype=torch.int64)
    dist.all_reduce(total)                      # host-side sum of the per-rank summaries (multicore.py:389)
    if rank == 0:
        open(path_out + ".total", "w").write(str(int(total.item())))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_trim_file_matches_single_process(tmp_path, emu_backend, world):
    """Each rank trims its own byte range of the FASTQ file; the parts in rank order are the
    single-process output (no data-path collective)."""
    import base64
    from atropos_amd.trim import pipeline_from_args
    from .conftest import load_golden
    data = base64.b64decode(load_golden("trim_cases.json.gz")["inputs"]["synth.fastq"])
    args = "-a AGATCGGAAGAGCACACGTCTGAACTCCAGTCA -q 20 --trim-n -m 20"
    path_in, path_out = str(tmp_path / "in.fastq"), str(tmp_path / "out.fastq")
    open(path_in, "wb").write(data)
    mp.spawn(_trim_worker, args=(world, _free_port(), path_in, path_out, args), nprocs=world, join=True)
    parts = b"".join(open("%s.part%d" % (path_out, r), "rb").read() for r in range(world))
    assert parts == pipeline_from_args(args).trim_bytes(data)
    assert int(open(path_out + ".total").read()) == data.count(b"\n") // 4


def test_fastq_shard_ranges_are_record_aligned(tmp_path):
    from atropos_amd.shard import fastq_shard_ranges
    recs = []
    for i in range(200):
        n = 10 + (i * 7) % 40
        q = ("@" + "I" * (n - 1)) if i % 3 == 0 else "I" * n       # quality lines that start with '@'
        recs.append("@r%d\n%s\n+\n%s\n" % (i, "A" * n, q))
    text = "".join(recs).encode()
    path = str(tmp_path / "x.fastq")
    open(path, "wb").write(text)
    for world in (1, 2, 3, 5, 8):
        ranges = fastq_shard_ranges(path, world)
        assert ranges[0][0] == 0 and ranges[-1][1] == len(text)
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        for lo, hi in ranges:
            shard = text[lo:hi]
            assert shard.count(b"\n") % 4 == 0
            assert not shard or shard.startswith(b"@r")


@pytest.mark.parametrize("world", [2, 3, 8])
def test_single_process_multi_device(emu_backend, world):
    """The single-process driver (one host thread + backend per device, one host result buffer at
    per-device offsets) equals the single-device run -- locate and the fused linked-adapter pipeline."""
    import numpy as np
    from atropos_amd import shard, synth
    from atropos_amd.adapters import AsciiSource, LinkedAdapter, LinkedSet, upper_ascii
    from atropos_amd.align import Aligner
    from tests.emu.backend import EmuBackend
    backends = [EmuBackend() for _ in range(world)]
    w = synth.workload("C2", 0, 1001)
    make = lambda: Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
    rec, seconds = shard.sharded_locate_threads(make, w["reads"], backends)
    assert len(seconds) == world and torch.equal(rec, make().locate_batch(w["reads"]).records)
    w4 = synth.workload("C4", 0, 777)
    reads = upper_ascii(w4["reads"])
    mk = lambda: LinkedSet([LinkedAdapter(f, b, front_anchored=True, back_anchored=False, max_error_rate=w4["max_error_rate"],
                                          min_overlap=w4["min_overlap"], indel_cost=w4["indel_cost"])
                            for f, b in zip(w4["fronts"], w4["backs"])])
    got, _ = shard.sharded_linked_threads(mk, reads, None, backends)
    which, count, front, back = mk().match_source(AsciiSource(reads))
    assert torch.equal(got[:, 0, 0].to(torch.int32), which) and torch.equal(got[:, 0, 1].to(torch.int32), count)
    assert torch.equal(got[:, 1], front) and torch.equal(got[:, 2], back)


def test_fastq_shard_ranges_monotone(tmp_path):
    """A probe that finds no record boundary must not make shards overlap (advisor finding)."""
    from atropos_amd import shard
    path = tmp_path / "long.fastq"
    rec = b"@r\n" + b"A" * 3_000_000 + b"\n+\n" + b"I" * 3_000_000 + b"\n"
    path.write_bytes(rec * 2)
    ranges = shard.fastq_shard_ranges(str(path), 4)
    assert ranges[0][0] == 0 and ranges[-1][1] == len(rec) * 2
    assert all(a <= b for a, b in ranges) and all(ranges[i][1] == ranges[i + 1][0] for i in range(3))


def _run_bench(cmd, env_extra):
    import json
    import subprocess
    env = dict(os.environ, ATROPOS_BENCH_BACKEND="emu", ATROPOS_BENCH_EMU_UNITS="1500", **env_extra)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    done = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    lines = [ln for ln in done.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), done.stdout.decode()[-2000:]   # ONE line on stdout: rank 0's JSON
    return json.loads(lines[0])


def _check_bench_line(line, world):
    assert line["n_gpus"] == world and line["steps"] == 2 and line["warmup"] == 1
    assert line["scaling"] == "weak" and line["config"]["parallelism"] == "shard%d" % world
    assert len(line["per_rank_ms_per_step"]) == world and all(t > 0 for t in line["per_rank_ms_per_step"])
    assert abs(line["ms_per_step"] - max(line["per_rank_ms_per_step"])) < 1e-9          # max over ranks
    units = line["config"]["reads_per_gpu"]
    assert abs(line["value"] - units * world * 2 / (line["ms_per_step"] * 2e-3)) < 1e-3 * line["value"]
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["achieved"] > 0 and len(roof["per_rank_kernel_ms"]) == world
    assert "gloo" in line["launcher"] and "no RCCL" in line["launcher"]
    for name in ("C3", "C4", "C5"):                                        # the other configs ride in the same line
        assert line["configs"][name]["n_gpus"] == world and "error" not in line["configs"][name]


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2 --steps S --warmup W --full` -- the driver's N = 1 command with N substituted and NO
    launcher around it -- must produce the 2-rank line by itself (round-3 verdict: it exited 1)."""
    line = _run_bench([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"], {})
    _check_bench_line(line, 2)
    assert "self-launch" in line["launcher"]


def test_bench_under_torch_distributed_run():
    """The driver's multi-GPU form: torch.distributed.run starts the ranks, bench.py reads RANK / WORLD_SIZE."""
    line = _run_bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                       "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
                       "--steps", "2", "--warmup", "1", "--full"], {})
    _check_bench_line(line, 2)
    assert "torch.distributed.run" in line["launcher"]


def test_bench_dump_outputs(tmp_path, oracle):
    """`bench.py --dump-outputs DIR`: every config's last-step outputs as float32 .npy files, the same from run to run,
    within 64 MB; C2's records are the oracle's on the batch the last timed step used (step warmup + steps - 1 of a
    rotation over three batches: batch 2, reads [2 n, 3 n) of the generator)."""
    import glob
    import numpy as np
    from atropos_amd import synth
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        line = _run_bench([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                           "--no-secondary", "--no-live-counters", "--dump-outputs", str(d)], {})
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        dumps.append({os.path.basename(p): np.load(p) for p in sorted(glob.glob(str(d / "*.npy")))})
        assert sum(os.path.getsize(p) for p in glob.glob(str(d / "*.npy"))) <= 64_000_000
    a, b = dumps
    assert sorted(a) == sorted(b) and {k.split("_")[0] for k in a} == {"C2", "C3", "C4", "C5"}
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    n = len(a["C2_records.npy"])
    assert n == 1500
    w = synth.workload("C2", 2 * n, n)
    reads = w["reads"].numpy()
    exp = oracle.locate_many(w["adapter"], reads, np.full(n, 150, np.int32), w["max_error_rate"], 14, False, False,
                             w["min_overlap"], w["indel_cost"], 2)
    assert np.array_equal(a["C2_records.npy"][:, :6], exp)


def test_bench_plain_run_reports_the_headline_only(tmp_path):
    """A plain `bench.py --gpus 1 --steps S --warmup W` reports C2 and nothing else: the headline fields, no other
    config, CPU baseline or side measurement; with --dump-outputs it writes the same files as a --full run."""
    import glob
    import numpy as np
    runs = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-secondary", "--no-live-counters"])):
        d = tmp_path / name
        line = _run_bench([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                           "--dump-outputs", str(d)] + extra, {})
        runs[name] = (line, {os.path.basename(p): np.load(p) for p in glob.glob(str(d / "*.npy"))})
    line, dump = runs["plain"]
    assert line["metric"] == "reads/s (whole node) 150 bp SE adapter-align" and line["unit"] == "reads/s"
    assert line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    units = line["config"]["reads_per_gpu"]
    assert abs(line["value"] - units / (line["ms_per_step"] * 1e-3)) < 1e-3 * line["value"]
    assert not {"configs", "cpu_baseline", "secondary"} & set(line)
    assert list(line["configs_summary"]) == ["C2"]
    full_line, full_dump = runs["full"]
    assert sorted(full_line["configs"]) == ["C3", "C4", "C5"]
    assert sorted(dump) == sorted(full_dump) and {k.split("_")[0] for k in dump} == {"C2", "C3", "C4", "C5"}
    for k in dump:
        assert np.array_equal(dump[k], full_dump[k]), k


def test_bench_scaling_curve_one_invocation():
    """`python bench.py --scaling`: the N = 1, 2, 4, 8 lines from ONE invocation (round-4 verdict, item 9) -- here on
    the CPU test double with ranks sharing the one 'device'; every line carries its per-rank times."""
    import json
    import subprocess
    env = dict(os.environ, ATROPOS_BENCH_BACKEND="emu", ATROPOS_BENCH_EMU_UNITS="600")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    done = subprocess.run([sys.executable, "bench.py", "--scaling", "--oversubscribe", "--steps", "2", "--warmup", "1"], cwd=ROOT,
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    lines = [json.loads(ln) for ln in done.stdout.decode().splitlines() if ln.strip().startswith("{")]
    assert [ln["n_gpus"] for ln in lines] == [1, 2, 4, 8]
    for ln in lines:
        assert len(ln["per_rank_ms_per_step"]) == ln["n_gpus"] and ln["scaling"] == "weak"
        assert abs(ln["ms_per_step"] - max(ln["per_rank_ms_per_step"])) < 1e-9
        if ln["n_gpus"] > 1:
            assert len(ln["roofline"]["per_rank_kernel_ms"]) == ln["n_gpus"]
