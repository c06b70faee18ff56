"""GPU (-m gpu): the N>1 path on real hardware -- RCCL (torch.distributed backend "nccl") initialised with however
many devices are visible, the HIP compress path on every rank's contiguous shard, the all-gather of the uint32
output lengths, checked against the oracle; plus bench.py's sharded entry (BASELINE configs[4]
shape, reduced) launched exactly as the driver launches it."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, nblocks, n, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        import hdl_deflate_amd
        from hdl_deflate_amd.data import make_blocks
        from hdl_deflate_amd.shard import LengthGather, shard_range, archive_offsets
        eng = hdl_deflate_amd.Engine(dev)
        b0, b1 = shard_range(nblocks, rank, world)
        d_in = make_blocks(b1 - b0, n, dev, seed=3, first_block=b0, chunk=4)
        out, ol, st = eng.compress_batch(d_in)
        lg = LengthGather(nblocks, dev)
        all_len = lg.gather(ol).clone()
        again = lg.gather(ol)                                   # buffers are reused: a second step gives the same
        offs, total = archive_offsets(all_len)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0 and torch.equal(all_len, again)
        assert torch.equal(all_len[b0:b1], ol)
        # the same exchange on a process group that is not the default one, and the payload gather (8(f) rank 2) on
        # RCCL -- a world of ONE rank goes through ncclAllGather too, so the first real multi-GPU run is not their first execution
        from hdl_deflate_amd.shard import gather_archive, gather_lengths
        grp = dist.new_group(ranks=list(range(world)))
        assert torch.equal(LengthGather(nblocks, dev, group=grp).gather(ol), all_len)
        assert torch.equal(gather_lengths(ol, nblocks, group=grp), all_len)
        arch, aoff = eng.compact(out, ol)
        nloc = int(ol.to(torch.int64).sum().item())
        whole = gather_archive(arch, nloc, group=grp)
        torch.cuda.synchronize()
        assert whole.numel() == total and torch.equal(whole[int(offs[b0]):int(offs[b0]) + nloc], arch[:nloc])
        q.put((rank, b0, d_in.cpu().numpy(), out.cpu().numpy(), all_len.cpu().numpy(), offs.cpu().numpy(), total))
    finally:
        dist.destroy_process_group()


def test_rccl_length_allgather_over_visible_devices(oracle):
    import torch
    import torch.multiprocessing as mp
    world = torch.cuda.device_count()
    assert world >= 1
    nblocks, n = 16 * world + (3 if world > 1 else 0), 4096     # uneven shards whenever there is more than one rank
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, world, port, nblocks, n, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=600) for _ in ps), key=lambda t: t[0])
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    want = []
    for rank, b0, h_in, h_out, all_len, offs, total in res:
        for k in range(h_in.shape[0]):
            rc, ref = oracle.compress(h_in[k].tobytes(), 32, 10)
            assert rc == 0 and h_out[k, :all_len[b0 + k]].tobytes() == ref, (rank, k)
            want.append(len(ref))
    for rank, b0, h_in, h_out, all_len, offs, total in res:      # every rank holds the whole job's lengths + offsets
        assert all_len.tolist() == want
        assert offs.tolist() == list(np.cumsum([0] + want[:-1])) and total == sum(want)


def _run_bench(world, env_extra, args):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(REPO, "bench.py"), "--gpus", str(world), "--detail", ""] + args
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    assert len(lines[0]) < 12288, len(lines[0])                  # (the driver did not parse a 20 KB line)
    return json.loads(lines[0])


def test_bench_sharded_entry_cfg5_shape():
    """bench.py --gpus N as the driver launches it (torch.distributed.run, one rank per GPU): the configs[4] shape,
    reduced to 2048 blocks; with a single visible device the same entry runs as two ranks sharing the GPU over gloo
    (the collective is then not RCCL -- the RCCL leg is the test above)"""
    import torch
    ndev = torch.cuda.device_count()
    args = ["--cfg5-blocks", "2048", "--steps", "2", "--warmup", "1"]
    if ndev > 1:
        r = _run_bench(ndev, {}, args)
    else:
        r = _run_bench(2, {"HDLZ_BENCH_BACKEND": "gloo"}, args)
    assert r["scaling"] == "strong" and r["n_gpus"] == max(ndev, 2) and r["value"] > 0
    assert r["config"]["blocks_total"] == 2048 and r["config"]["block_bytes"] == 65536
    assert 0.3 < r["compression_ratio_out_over_in"] < 0.8 and r["roofline"]["frac"] > 0


def test_bench_gpus_n_without_a_launcher():
    """`python3 bench.py --gpus N` started plainly (the form the driver uses for N = 1) starts its own N ranks.
    With one visible device: over RCCL it must say so in ONE JSON line and exit non-zero instead of hanging or asserting; the
    functional flow (ranks sharing the device over gloo) must produce the line with T1_ms in it."""
    import torch
    ndev = torch.cuda.device_count()
    n = max(2, ndev)
    base = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(n), "--cfg5-blocks", "2048", "--steps", "2", "--warmup", "1", "--detail", ""]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HDLZ_BENCH_BACKEND")}
    if ndev < n:
        p = subprocess.run(base, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert p.returncode != 0 and len(lines) == 1, p.stdout[-2000:] + p.stderr[-2000:]
        r = json.loads(lines[0])
        assert r["value"] is None and r["visible_devices"] == ndev and "error" in r
        env["HDLZ_BENCH_BACKEND"] = "gloo"
    p = subprocess.run(base, cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == n and r["scaling"] == "strong" and r["value"] > 0 and r["config"]["blocks_total"] == 2048
    assert r["T1_ms"] > 0 and r["speedup_vs_T1"] > 0 and r["roofline"]["kernel_ms_median"] > 0


def test_shards_of_any_world_size_hold_the_single_gpu_jobs_bytes():
    """block contents depend on (seed, global block index) only -- uneven shards (world 3, 5, 7) and any chunk
    grid give exactly the bytes of the one-GPU job"""
    import torch
    from hdl_deflate_amd.data import make_blocks
    from hdl_deflate_amd.shard import shard_range
    whole = make_blocks(203, 4096, "cuda", seed=0)
    for world in (2, 3, 5, 7):
        parts = [make_blocks(b1 - b0, 4096, "cuda", seed=0, first_block=b0, chunk=5 + world)
                 for b0, b1 in (shard_range(203, r, world) for r in range(world))]
        assert torch.equal(torch.cat(parts), whole), world


def test_bench_gpus_8_even_and_uneven_jobs():
    """`bench.py --gpus 8` end to end on the job shapes of BASELINE configs[4] (blocks / 8 per rank) and on an UNEVEN job
    (three ranks hold one block more): eight ranks -- over RCCL when eight devices are visible, else sharing the visible device(s) over
    gloo --, the gathered lengths asserted equal to the 1-rank job's INSIDE the run (byte count + position-weighted digest, T1 leg)"""
    import torch
    ndev = torch.cuda.device_count()
    env = {} if ndev >= 8 else {"HDLZ_BENCH_BACKEND": "gloo"}
    for blocks in (1024, 1027):
        r = _run_bench(8, env, ["--cfg5-blocks", str(blocks), "--steps", "2", "--warmup", "1"])
        assert r["n_gpus"] == 8 and r["scaling"] == "strong" and r["value"] > 0 and r["config"]["blocks_total"] == blocks
        assert r["config"]["blocks_per_gpu"] == blocks // 8 + (1 if blocks % 8 else 0)          # rank 0's shard
        assert r["lengths_digest"] == r["T1_lengths_digest"] and r["T1_ms"] > 0


def test_bench_single_gpu_line_is_short_and_complete(tmp_path):
    """the `--gpus 1` line (every secondary entry, reduced sizes) is ONE line below 12 KB that carries the contract's
    keys, `roofline` and `cpu_baseline`; the prose went to the detail file it names"""
    detail = str(tmp_path / "bench_detail.json")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--full", "--blocks", "65536", "--cfg5-blocks", "2048", "--text-blocks", "256",
           "--streams", "65536", "--steps", "2", "--warmup", "1", "--cpu-seconds", "1", "--detail", detail]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 12288, [len(ln) for ln in lines]
    r = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "secondary", "detail"):
        assert k in r, k
    assert r["n_gpus"] == 1 and r["value"] > 0 and r["roofline"]["frac"] > 0 and r["roofline"]["bound"] == "hbm"
    assert r["cpu_baseline"]["kind"] == "port" and r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["cores"] >= 1
    assert len(r["secondary"]) >= 9 and all(e["value"] > 0 and e["roofline"]["frac"] > 0 for e in r["secondary"])
    full = json.load(open(detail))
    assert full["value"] == r["value"] and "note" in full["roofline"] and len(full["secondary"]) == len(r["secondary"])


def test_bench_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    """a plain `--gpus 1` run: the headline line alone (no roofline, cpu_baseline, secondary entries or detail file), the steps asked
    for; --dump-outputs writes what the last timed step returned -- the same arrays in two runs with the same arguments, and the
    sampled rows are zlib streams of the benchmark's blocks"""
    import zlib
    import torch
    from hdl_deflate_amd.data import make_blocks
    B, n = 65536, 2048
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    runs = []
    for k in range(2):
        d = tmp_path / ("dump%d" % k)
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--blocks", str(B), "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(d)]
        p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        r = json.loads(lines[0])
        assert r["metric"] == "compress_input_throughput (CWINDOW=32, MATCH10=True, static tree)" and r["unit"] == "MB/s"
        assert r["higher_is_better"] is True and r["dtype"] == "u8" and r["steps"] == 3 and r["warmup"] == 1
        assert r["value"] > 0 and abs(r["value"] - B * n / (r["ms_per_step"] * 1e3)) <= 0.01 * r["value"]
        for key in ("roofline", "cpu_baseline", "secondary", "archive", "end_to_end", "detail"):
            assert key not in r, key
        runs.append({f: np.load(str(d / f)) for f in ("out_len.npy", "status.npy", "out_rows_sample.npy")})
    for f in runs[0]:
        assert runs[0][f].dtype in (np.float32, np.float64) and np.array_equal(runs[0][f], runs[1][f]), f
    ol, st, rows = runs[0]["out_len.npy"], runs[0]["status.npy"], runs[0]["out_rows_sample.npy"]
    assert ol.shape == (B,) and (st == 0).all() and rows.shape[0] == 4096 and sum(a.nbytes for a in runs[0].values()) < 64e6
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    idx = torch.randperm(B, generator=g)[:rows.shape[0]].sort().values
    blocks = make_blocks(B, n, "cuda", seed=0)[idx.cuda()].cpu().numpy()
    for k in range(0, rows.shape[0], 97):
        L = int(ol[idx[k]])
        assert not rows[k, L:].any()
        assert zlib.decompress(rows[k, :L].astype(np.uint8).tobytes()) == blocks[k].tobytes(), k
