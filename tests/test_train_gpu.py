"""GPU: train-step parity vs the oracle (one full optimisation step incl. clip + AdamW), short training run,
checkpoint -> inference round trip through the entry points."""
import os

import pytest
import torch

from oracle import bsrnn_ref, losses_ref

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from urgent2026_challenge_track1_amd.config import Config
    base = dict(model_configs={"num_channel": 16, "num_layer": 1}, compute_dtype="f32", seed=7, batch_size=2,
                num_worker=0, train_set_path="synthetic:8", valid_set_path="synthetic", val_check_interval=3,
                num_train_epochs=2, save_top_k=1, resume=False)
    base.update(kw)
    return Config(**base)


def test_two_optimisation_steps_match_oracle(lib):
    """SEModel.training_step + backward + clip 0.5 + AdamW for two steps == oracle train_step (f32)."""
    from urgent2026_challenge_track1_amd.d_model import SEModel
    torch.manual_seed(3)
    ref = bsrnn_ref.BSRNN_SE(16, 1)
    opt_r = losses_ref.make_optimizer(ref.parameters())
    model = SEModel(_cfg())
    model.se_model.load_state_dict(ref.state_dict())
    model = model.cuda()
    (opt,), _ = model.configure_optimizers()
    g = torch.Generator().manual_seed(5)
    for it in range(2):
        clean = 0.3 * torch.randn(2, 1, 3200, generator=g)
        noisy = clean + 0.1 * torch.randn(2, 1, 3200, generator=g)
        lens = torch.tensor([3200, 3200], dtype=torch.int32)
        fs = torch.tensor(16000, dtype=torch.int32)
        loss_r, sisnr_r, gn_r = losses_ref.train_step(ref, opt_r, clean, noisy, 16000, lens)
        loss = model.training_step((clean.cuda(), noisy.cuda(), fs, lens))
        loss.backward()
        model.optimizer_step(opt)
        assert abs(float(loss) - float(loss_r)) <= 1e-3 * abs(float(loss_r)), it
        assert abs(float(model.logged["train_sisnr"]) - float(sisnr_r)) <= 1e-2
        assert abs(float(model.logged["Grad_norm"]) - float(gn_r)) <= 1e-3 * float(gn_r)
    # Adam's first steps are sign descent (m/sqrt(v) = +-1): an element whose gradient is ~0 can flip sign on a 1e-9
    # difference and then differs by 2*lr per step.  So: almost all elements agree tightly, none differs by more than
    # 2*lr*steps, and the aggregate update agrees.
    tot = bad = 0
    refp = dict(ref.named_parameters())
    for n, p in model.se_model.named_parameters():
        d = (p.detach().cpu() - refp[n].detach()).abs()
        assert d.max().item() <= 2 * 1e-3 * 2 + 1e-5, n
        tot += d.numel()
        bad += int((d > 2e-5).sum())
    assert bad <= 1e-3 * tot, (bad, tot)


def test_fit_checkpoint_inference_roundtrip(lib, tmp_path):
    from urgent2026_challenge_track1_amd import inference, train_se
    from urgent2026_challenge_track1_amd.dataset import SyntheticPairDataset, read_audio, write_audio
    os.chdir(tmp_path)
    cfg = _cfg(train_tag="t", train_name="n")
    model, steps = train_se.fit(cfg, max_steps=4, log_every=2)
    assert steps == 4
    ck = [f for f in os.listdir(train_se.ckpt_dir(cfg)) if "val_loss" in f]
    assert len(ck) == 1
    ds = SyntheticPairDataset(1, fs_list=(16000,), seconds=0.5)
    clean, noisy, fs, L = ds[0]
    write_audio(str(tmp_path / "in.wav"), noisy[0], fs, "FLOAT")
    x, fs2 = read_audio(str(tmp_path / "in.wav"))
    assert fs2 == fs and abs(x - noisy).max() == 0
    (tmp_path / "in.scp").write_text("utt1 %s\n" % (tmp_path / "in.wav"))
    args = inference.parser().parse_args(["--input_scp", str(tmp_path / "in.scp"), "--output_dir", str(tmp_path / "out"),
                                          "--ckpt_path", os.path.join(train_se.ckpt_dir(cfg), ck[0])])
    inference.main(args)
    y, fs3 = read_audio(str(tmp_path / "out" / "wav" / "utt1.wav"))
    assert fs3 == fs and y.shape[1] == L and abs(abs(y).max() - 0.9) < 1e-3
    assert (tmp_path / "out" / "inf.scp").read_text().split()[0] == "utt1"


def test_two_ranks_on_one_gpu_hold_identical_weights(lib):
    """the N > 1 path of bench.py (broadcast, bucketed all-reduce driven by the backward's ready tags, deferred wgrads on
    the second queue) with two gloo ranks sharing cuda:0 and different data per rank: after the steps both hold the same
    weights bit for bit"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29531", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--dist-backend", "gloo", "--pretouch-gib", "0", "--batch", "2", "--seconds", "1", "--channels", "32", "--layers", "2"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["ranks_hold_identical_weights"] is True
    assert d["config"]["global_batch"] == 4


def test_bench_gpus_2_starts_its_own_ranks(lib):
    """`python bench.py --gpus 2` with NO torchrun in the command: the parent starts the two ranks itself (child process group),
    relays rank 0's line, and the line says n_gpus 2 (--gpus was parsed and never read).  gloo lets both ranks share
    the one GPU of this box; `--dynamic-mix` puts config C3's on-GPU simulator feed into the N > 1 step."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--dist-backend", "gloo",
           "--pretouch-gib", "0", "--batch", "2", "--seconds", "1", "--channels", "32", "--layers", "2", "--dynamic-mix"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["ranks_hold_identical_weights"] is True and d["config"]["dist_backend"] == "gloo"
    assert d["config"]["global_batch"] == 4 and "dynamic_mix" in d


@pytest.mark.gpu
def test_single_rank_rccl_carries_the_gradient_buckets(lib, tmp_path):
    """The RCCL leg of the N > 1 step on a 1-GPU box: `--single-rank-collectives` creates the `nccl` (= RCCL) process group with one
    rank and sends the weight broadcast, every gradient bucket (async, on the reducer's stream, beside the backward's kernels), the
    barriers and the checksum reductions through it.  The step must issue one collective per bucket and step, end with the loss
    the plain one-GPU run ends with, and the line must say backend nccl.  (Two RCCL ranks cannot share a device; the two-rank
    arithmetic is covered over gloo above.)  Both runs write what their last timed step computed (--dump-outputs)."""
    import json, os, subprocess, sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NCCL_MAX_NCHANNELS")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pretouch-gib", "0",
            "--batch", "2", "--seconds", "1", "--channels", "32", "--layers", "2", "--no-flow", "--no-metrics", "--no-cpu-baseline", "--no-dist-leg"]
    lines = []
    for i, extra in enumerate(([], ["--single-rank-collectives", "--dist-backend", "nccl"])):
        r = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / str(i))], cwd=root, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    plain, rccl = lines
    dumps = [{k: np.load(tmp_path / str(i) / (k + ".npy")) for k in ("loss", "sisnr", "grad_norm", "weights")} for i in range(2)]
    for d, line in zip(dumps, lines):
        assert float(d["loss"]) == line["final_loss"] and d["loss"].dtype == np.float32, (float(d["loss"]), line["final_loss"])
        assert np.isfinite(d["sisnr"]) and d["grad_norm"] > 0 and d["weights"].dtype == np.float32 and np.isfinite(d["weights"]).all()
    assert dumps[0]["weights"].shape == dumps[1]["weights"].shape
    assert plain["config"]["dist_backend"] is None and "gradient_buckets" not in plain
    assert rccl["config"]["dist_backend"] == "nccl" and rccl["n_gpus"] == 1 and rccl["ranks_hold_identical_weights"] is True
    gb = rccl["gradient_buckets"]
    assert gb["buckets"] >= 1 and gb["collectives_issued"] == gb["buckets"] * 4          # 1 warm-up + 3 timed steps
    # (the weight-gradient GEMMs sum their K slices with f32 atomics, so two runs agree to rounding, not bit for bit)
    assert abs(rccl["final_loss"] - plain["final_loss"]) <= 1e-3 * abs(plain["final_loss"]), (rccl["final_loss"], plain["final_loss"])


def test_cooperative_bptt_beside_rccl_buckets_leaves_the_collective_its_cus(lib, tmp_path):
    """the flow model's backward runs the COOPERATIVE split BPTT (every workgroup must be resident) while the
    reducer's all-reduce kernels occupy CUs.  From the first bucket to finish() `ops.reserved_cus()` includes RCCL's channel cap
    (NCCL_MAX_NCHANNELS is capped before the communicator exists), so the split kernel is planned on the remaining CUs or refused
    (counted) - never launched on a grid that cannot be co-resident.  Run: BSRNN-Flow C4 train steps through a single-rank RCCL group,
    which also writes what its last timed step and the sampler computed (--dump-outputs)."""
    import json, os, subprocess, sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NCCL_MAX_NCHANNELS")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--model", "flow", "--gpus", "1", "--steps", "2", "--pretouch-gib", "0",
           "--single-rank-collectives", "--dist-backend", "nccl", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    fb = line["flow_c4"]
    assert "error" not in fb, fb
    co = fb["cooperative_kernels_beside_rccl"]
    assert co["kernel_error_flag"] == 0, co
    assert co["reserved_cus_during_backward"] == 32 and co["reserved_cus_after_step"] == 0, co
    assert co["collectives_issued"] == co["buckets"] * 3 and co["buckets"] >= 2, co          # 1 warm-up + 2 timed steps
    # the cooperative kernel ran (on a smaller plan) or was refused and replaced by the streaming BPTT - either way every BPTT launched
    lc = co["launch_counts"]
    assert lc.get("lstm_bwd_split", 0) + lc.get("lstm_bwd_stream16", 0) + lc.get("lstm_bwd_stream32", 0) > 0, co
    assert fb["final_loss"] == fb["final_loss"]
    d = {k: np.load(tmp_path / (k + ".npy")) for k in ("loss", "weights", "enhanced", "enhanced_f16")}
    assert float(d["loss"]) == fb["final_loss"] and d["weights"].shape == (1 << 22,), (float(d["loss"]), d["weights"].shape)
    assert d["enhanced"].size == d["enhanced_f16"].size == 192000 and np.isfinite(d["enhanced"]).all(), d["enhanced"].shape


@pytest.mark.gpu
def test_full_size_c2_step_as_one_rccl_rank_runs_the_cooperative_kernels_beside_the_buckets(lib):
    """VERDICT r5 item 1 (reference `baseline_code/train_se.py:74-83`, Lightning DDP): what ONE rank of a DDP job runs, at the size
    bench.py times (B 32 x 4 s @ 48 kHz, N 196, 6 layers) - the step as the only rank of an RCCL process group.  Every gradient bucket is
    all-reduced on the reducer's stream beside the backward; from the first bucket to finish() `ops.COMM_RESERVED_CUS` = the RCCL
    channel cap, and the N-split BPTT (H 392; pairs of workgroups that spin for each other) is planned on the CUs that leaves, next
    to the second queue's weight-gradient workgroups.  The fused cluster forward runs outside that window (no bucket in flight).
    Asserted: both cooperative kernels ran (or every missing one is explained by a counted refusal), the bounded spins never tripped
    the device error flag, one collective per bucket and step, and the loss after the steps is the plain run's."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NCCL_MAX_NCHANNELS")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pretouch-gib", "0",
            "--no-flow", "--no-metrics", "--no-cpu-baseline", "--no-f32-mode", "--no-dist-leg"]
    lines = []
    for extra in ([], ["--single-rank-collectives", "--dist-backend", "nccl"]):
        r = subprocess.run(base + extra, cwd=root, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    plain, rccl = lines
    assert "B32 x 4 s" in rccl["config"]["workload"] and "N=196 L=6" in rccl["config"]["workload"]
    assert rccl["config"]["dist"]["backend"] == "nccl" and rccl["config"]["dist"]["world_size"] == 1
    co = rccl["cooperative_kernels_beside_rccl"]
    lc = co["launch_counts"]
    assert co["kernel_error_flag"] == 0, co
    assert co["reserved_cus_during_backward"] == rccl["config"]["dist"]["comm_reserved_cus"] == 32 and co["reserved_cus_after_step"] == 0, co
    # 6 layers x 2 directions are one launch each: 6 per step, 4 steps (1 warm-up + 3 timed) - or a counted refusal per missing launch
    # (forward: no bucket in flight, nothing reserved - the time path in one round and, round 6, the band path in 12 rounds: 12 launches per step)
    assert lc.get("lstm_fwd_clusterx", 0) == 48, co
    assert lc.get("lstm_bwd_nsplit", 0) + co["plans_refused"] >= 24 and lc.get("lstm_bwd_nsplit", 0) > 0, co
    gb = rccl["gradient_buckets"]
    assert gb["buckets"] >= 4 and gb["collectives_issued"] == gb["buckets"] * 4, gb
    assert rccl["ranks_hold_identical_weights"] is True
    assert abs(rccl["final_loss"] - plain["final_loss"]) <= 1e-3 * abs(plain["final_loss"]), (rccl["final_loss"], plain["final_loss"])
    os.makedirs(os.path.join(root, "gpurun_out", "parity"), exist_ok=True)
    with open(os.path.join(root, "gpurun_out", "parity", "c2_one_rccl_rank.json"), "w") as f:
        json.dump({"plain_ms_per_step": plain["ms_per_step"], "rccl_rank_ms_per_step": rccl["ms_per_step"],
                   "plain_final_loss": plain["final_loss"], "rccl_final_loss": rccl["final_loss"],
                   "gradient_buckets": gb, "cooperative_kernels_beside_rccl": co, "dist": rccl["config"]["dist"]}, f, indent=1)


def test_inference_half_default_on_a_trained_checkpoint_validated_and_with_a_way_back(lib, tmp_path, monkeypatch):
    """`inference.load_from_checkpoint` enhances a bf16-trained checkpoint with IEEE-half operands by default.
    (a) on a checkpoint that HAS been trained (40 optimisation steps in bf16 through train_se.fit: weights that left their initialisation)
    the f16 waveform stays within 1e-3 of the f32-mode waveform of the same checkpoint, the bf16 one does not need to;
    (b) an unknown URSE_INFER_DTYPE is a ValueError that names the choices, not a KeyError;
    (c) half has a range of 65504: a checkpoint whose activations leave it (weights scaled up here) gives a non-finite waveform, which
    enhance_file notices and answers by re-running the utterance in the checkpoint's own operand type, with a warning."""
    import warnings
    from urgent2026_challenge_track1_amd import inference, train_se
    from urgent2026_challenge_track1_amd.dataset import SyntheticPairDataset
    os.chdir(tmp_path)
    cfg = _cfg(train_tag="h", train_name="n", compute_dtype="bf16", model_configs={"num_channel": 32, "num_layer": 2},
               train_set_path="synthetic:16", val_check_interval=40, num_train_epochs=5)
    model, steps = train_se.fit(cfg, max_steps=40, log_every=20)
    assert steps == 40
    ck = [f for f in os.listdir(train_se.ckpt_dir(cfg)) if "val_loss" in f]
    path = os.path.join(train_se.ckpt_dir(cfg), ck[0])
    _, noisy, fs, L = SyntheticPairDataset(1, fs_list=(48000,), seconds=1.0)[0]
    outs = {}
    for want in ("f32", "f16", "bf16"):
        monkeypatch.setenv("URSE_INFER_DTYPE", want)
        m = inference.load_from_checkpoint(path)
        m.eval()
        assert m._ckpt_dtype == torch.bfloat16
        outs[want] = inference.enhance_file(m, noisy[0], fs, "cuda").cpu()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    print("trained checkpoint, 1 s @ 48 kHz: f16 vs f32 mode %.2e, bf16 vs f32 mode %.2e" % (rel(outs["f16"], outs["f32"]), rel(outs["bf16"], outs["f32"])))
    assert rel(outs["f16"], outs["f32"]) <= 1e-3
    assert rel(outs["f16"], outs["f32"]) < rel(outs["bf16"], outs["f32"])
    monkeypatch.setenv("URSE_INFER_DTYPE", "fp16")
    with pytest.raises(ValueError, match="bf16, f16, f32"):
        inference.load_from_checkpoint(path)
    monkeypatch.delenv("URSE_INFER_DTYPE")
    m = inference.load_from_checkpoint(path)
    m.eval()
    core = m.se_model.core
    assert core.compute_dtype == torch.float16
    with torch.no_grad():
        for n, p in m.se_model.named_parameters():
            if "fc" in n and "band_split" in n and n.endswith("weight"):
                p.mul_(3e5)                     # band-split outputs ~1e5 x their trained scale: beyond half's range, far inside bf16's
        core.param_version += 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        y = inference.enhance_file(m, noisy[0], fs, "cuda")
    assert any("checkpoint's own operand type" in str(x.message) for x in w), [str(x.message) for x in w]
    assert core.compute_dtype == torch.bfloat16 and bool(torch.isfinite(y).all())


@pytest.mark.gpu
def test_default_bench_line_carries_the_one_rccl_rank_leg(lib):
    """`python bench.py` (no --no-dist-leg): after the timed steps the parent starts the SAME workload once more as the only rank of an RCCL process
    group (child process, timeout) and reports it under `config.dist`: `reserved_step_ms`, its ratio to the plain step, the buckets, the
    cooperative kernels' error flag and refusals.  Toy size here; the full-size figures are in the driver's line."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NCCL_MAX_NCHANNELS")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pretouch-gib", "0", "--batch", "2", "--seconds", "1",
           "--channels", "32", "--layers", "2", "--no-flow", "--no-metrics", "--no-cpu-baseline", "--no-f32-mode"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    dist = d["config"]["dist"]
    assert "error" not in dist, dist
    assert d["config"]["dist_backend"] is None                      # the headline run itself used no process group
    assert dist["backend"] == "nccl" and dist["world_size"] == 1 and dist["comm_reserved_cus"] == 32
    assert dist["reserved_step_ms"] > 0 and abs(dist["reserved_vs_plain"] - dist["reserved_step_ms"] / d["ms_per_step"]) < 1e-9
    assert dist["kernel_error_flag"] == 0 and dist["ranks_hold_identical_weights"] is True
    gb = dist["gradient_buckets"]
    assert gb["collectives_issued"] == gb["buckets"] * (3 + 2)        # 3 timed + 2 warm-up steps of the leg
