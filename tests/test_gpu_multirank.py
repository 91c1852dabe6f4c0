"""The product's multi-rank code with TWO ranks running the HIP kernels (VERDICT r03
"what's missing" 2): two freshly spawned processes (start_method "spawn", as bench.py and
codenerf.train.launch start ranks) form a world-size-2 gloo group, both on the test box's one GPU
(RCCL refuses two ranks on one device; on a node every rank has its own GPU and the group is RCCL).
This torch build's gloo takes device tensors in every collective the product uses (tools/gloo_probe.py,
profiles/r04/gloo_probe.jsonl), so the product code runs unchanged on the gloo group.

(a) parallel_image_render (nerf/__init__.py:137-226) of C4 chairs with 2 ranks: rank 0's gathered
    image vs the reference's 2-rank image (render_chairs.npz ``n2_rgb``) at 1e-4;
(b) two ranks each run train_minibatch (train.py:96-114) on their own 4096-ray chunk, with the flat
    gradient all-reduce (AdamW.allreduce_grads, DDP's average, util.py:139-142): both end with the same
    parameters, bit-identical to one process that averages the two chunks' gradients before ONE step;
(c) bench.py at 2 ranks (--backend gloo): gather_views + multi_rank_check -> multi_rank_maxdiff == 0,
    including 3 ranks, whose 5461-ray slices need the per-view chunk restart.
"""
import json
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _spawn(fn, world, *args):
    import torch.multiprocessing as mp
    from conftest import rendezvous
    mp.start_processes(fn, args=(world, rendezvous()) + args, nprocs=world, join=True, start_method="spawn")


def _init(rank, world, rdv):
    import torch.distributed as dist
    import codenerf
    dist.init_process_group("gloo", init_method=rdv, rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    codenerf.load_library()
    return dev


def _chairs_worker(rank, world, rdv, out_path):
    import torch.distributed as dist
    from codenerf import synthetic
    from codenerf.nerf import PointSampler, RaySampler, parallel_image_render
    from test_gpu_configs import model_from
    from test_gpu_parity import load
    from test_gpu_train import embedders
    dev = _init(rank, world, rdv)
    try:
        g = load("render_chairs.npz", dev)
        rs = RaySampler(128, 128, g["intrinsics"].cpu(), sample_size=4096, device=dev, datatype=torch.float32)
        ps = PointSampler(32, 128, 1.25, 2.75, "lindepth", False, torch.float32, dev)
        models = {"nerf_coarse": model_from(dev, synthetic.codenerf_params(0), "f32"),
                  "nerf_fine": model_from(dev, synthetic.codenerf_params(1), "f32")}
        cfg = NS(is_distributed=True, gpus=world, nerf=NS(validation=NS(chunksize=4096)))
        rgb = parallel_image_render(cfg, g["pose"], [g["z_s"], g["z_t"]], models, (rs, ps), embedders(dev), dev)
        if rank == 0:
            torch.save({"rgb": rgb.cpu()}, out_path)
        else:
            assert rgb is None
    finally:
        dist.destroy_process_group()


def test_parallel_image_render_two_ranks(tmp_path):
    from conftest import GOLDEN, margin
    import numpy as np
    out = str(tmp_path / "chairs.pt")
    _spawn(_chairs_worker, 2, out)
    rgb = torch.load(out, weights_only=True)["rgb"]
    ref = torch.from_numpy(np.load(os.path.join(GOLDEN, "render_chairs.npz"))["n2_rgb"])
    assert rgb.shape == ref.shape == (128 * 128, 3)
    margin("chairs_c4_two_processes[f32]", "rgb_f gathered", (rgb.double() - ref.double()).abs().max().item(), 1e-4)


def _chunk(dev, n, seed):
    g = torch.Generator().manual_seed(seed)
    ro = (torch.randn(n, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.3])).to(dev)
    rd = (torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])).to(dev)
    ids = torch.full((n,), 1, dtype=torch.int64, device=dev)
    return ro, rd, ids, torch.rand(n, 4, generator=g).to(dev)


def _setup(dev, distributed):
    from codenerf import train as T
    from codenerf.nerf import PointSampler
    from test_gpu_train import _opt_cfg, _train_models
    torch.manual_seed(0)
    models = _train_models(dev, 3)
    cfg = _opt_cfg()
    cfg.is_distributed = distributed
    opt, sched = T.prepare_optimizer(cfg, models)
    ps = PointSampler(64, 64, 0.8, 1.8, spacing_mode="lindepth", perturb=False, dtype=torch.float32, device=dev)
    return models, opt, sched, ps


def _train_worker(rank, world, rdv, out_dir):
    import numpy as np
    import torch.distributed as dist
    from codenerf import train as T
    from test_gpu_train import embedders
    dev = _init(rank, world, rdv)
    try:
        models, opt, sched, ps = _setup(dev, True)
        if rank == 1:       # a different start on rank 1: prepare_optimizer's broadcast must undo it
            with torch.no_grad():
                models["nerf_fine"].fc_rgb.weight.add_(1.0)
        opt.broadcast_params(0)
        # the bucketed reduction (the two MLPs' gradients start during the backward, AdamW.allreduce_begin) on
        # this gloo group too: the sums must be those of the one all-reduce
        opt.bucket_backends = ("nccl", "gloo")
        began = []
        real_begin = opt.allreduce_begin
        opt.allreduce_begin = lambda *a, **k: began.append(real_begin(*a, **k)) or began[-1]
        ro, rd, ids, tgt = _chunk(dev, 4096, 10 + rank)
        ids._cn_host_ids = np.full(ids.shape[0], 1, dtype=np.int64)   # as train_iteration hands them over
        for _ in range(2):
            T.train_minibatch(models, opt, sched, ps, embedders(dev), ro, rd, ids, tgt, 1e-5, is_distributed=True)
        torch.cuda.synchronize()
        assert began == [True, True], began
        torch.save({f"{k}.{n}": p.detach().cpu() for k, m in models.items() for n, p in m.named_parameters()},
                   os.path.join(out_dir, f"params{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _nosync_worker(rank, world, rdv, out_dir):
    """train_minibatch on 2 gloo ranks under torch's sync debug mode "error": the product code between
    the collectives must not synchronise (gloo itself stages device tensors through the host, so the
    mode is lifted for the duration of its all-reduce only)."""
    import numpy as np
    import torch.distributed as dist
    from codenerf import train as T
    from test_gpu_train import embedders
    dev = _init(rank, world, rdv)
    try:
        models, opt, sched, ps = _setup(dev, True)
        opt.broadcast_params(0)
        e = embedders(dev)
        chunks = []
        for k in range(3):
            ro, rd, ids, tgt = _chunk(dev, 4096, 20 + 2 * k + rank)
            ids._cn_host_ids = np.full(ids.shape[0], 1, dtype=np.int64)
            chunks.append((ro, rd, ids, tgt))
        T.train_minibatch(models, opt, sched, ps, e, *chunks[0], 1e-5, is_distributed=True)
        torch.cuda.synchronize()
        real = dist.all_reduce
        calls = []

        def gloo_all_reduce(*a, **k):
            calls.append(a[0].numel())
            torch.cuda.set_sync_debug_mode(0)
            try:
                return real(*a, **k)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        dist.all_reduce = gloo_all_reduce
        torch.cuda.set_sync_debug_mode("error")
        try:
            for c in chunks[1:]:
                T.train_minibatch(models, opt, sched, ps, e, *c, 1e-5, is_distributed=True)
        finally:
            torch.cuda.set_sync_debug_mode(0)
            dist.all_reduce = real
        torch.cuda.synchronize()
        assert len(calls) == 2, calls                          # ONE collective per optimiser step
        torch.save({f"{k}.{n}": p.detach().cpu() for k, m in models.items() for n, p in m.named_parameters()},
                   os.path.join(out_dir, f"nosync{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_train_minibatch_two_ranks_no_host_sync(tmp_path):
    """the per-step has-grad read-back is gone from AdamW.allreduce_grads."""
    _spawn(_nosync_worker, 2, str(tmp_path))
    got = [torch.load(str(tmp_path / f"nosync{r}.pt"), weights_only=True) for r in range(2)]
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), ("ranks differ", k)


def test_train_allreduce_two_ranks(tmp_path):
    """Two data-parallel chunk steps on 2 ranks vs one process averaging both chunks' gradients; the ranks
    reduce in two buckets (the MLPs' gradients started during the backward, then the rest)."""
    from codenerf import train as T
    from test_gpu_train import embedders
    _spawn(_train_worker, 2, str(tmp_path))
    got = [torch.load(str(tmp_path / f"params{r}.pt"), weights_only=True) for r in range(2)]
    dev = torch.device("cuda", 0)
    models, opt, sched, ps = _setup(dev, False)
    chunks = [_chunk(dev, 4096, 10 + r) for r in range(2)]
    keep = NS(step=lambda: None)
    for _ in range(2):
        grads = []
        opt.step = lambda closure=None: None             # capture each chunk's gradients, no update
        for ro, rd, ids, tgt in chunks:
            T.train_minibatch(models, opt, keep, ps, embedders(dev), ro, rd, ids, tgt, 1e-5)
            opt._sync_grads()
            grads.append(opt.flat_buffers()["grad"].clone())
        del opt.step
        flat = opt.flat_buffers()["grad"]
        flat.copy_(grads[0] + grads[1])                   # gloo SUM, then / world (AdamW.allreduce_grads)
        flat.div_(2)
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    want = {f"{k}.{n}": p.detach().cpu() for k, m in models.items() for n, p in m.named_parameters()}
    for k in want:
        assert torch.equal(got[0][k], got[1][k]), ("ranks differ", k)
        assert torch.equal(got[0][k], want[k]), ("vs the averaged single process", k)


_BENCH_HEADLINE = ["--steps", "2", "--warmup", "1", "--images-per-step", "2", "--no-extras"]


def _bench_worker(rank, world, rdv, out_dir, argv=_BENCH_HEADLINE):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      CODENERF_INIT_METHOD=rdv)
    sys.path.insert(0, ROOT)
    import bench
    # --full: the gather check and the side lines these tests read are not part of a plain run
    res = bench.run(bench.parse_args(list(argv) + ["--full", "--no-cpu-baseline", "--backend", "gloo", "--quiet"]))
    if rank == 0:
        with open(os.path.join(out_dir, "bench.json"), "w") as f:
            json.dump(res, f)


@pytest.mark.parametrize("world", [2, 3])
def test_bench_gather_views_multi_rank(tmp_path, world):
    """bench.py's N-rank headline: every view split over the ranks (Q5), rendered with per-view
    chunking, gathered (gather_views) -- view 0 equals the same view rendered in one process with
    the same split and chunking, bit for bit."""
    from conftest import margin
    _spawn(_bench_worker, world, str(tmp_path))
    res = json.load(open(tmp_path / "bench.json"))
    assert res["n_gpus"] == world and res["value"] > 0
    margin(f"bench_multi_rank_n{world}[f32]", "multi_rank_maxdiff", res["multi_rank_maxdiff"], 0.0)


def test_bench_eval_sharded_two_ranks(tmp_path):
    """bench.py's side lines at 2 ranks, with the ray-sharded C5 line (eval_c5_sharded: one optimisation,
    its 2048 rays per iteration split over the ranks) beside the per-rank C5 lines."""
    _spawn(_bench_worker, 2, str(tmp_path), ["--steps", "1", "--warmup", "0", "--images-per-step", "1",
                                              "--eval-iters", "2", "--train-iters", "0"])
    res = json.load(open(tmp_path / "bench.json"))
    sh = res["eval_c5_sharded"]
    assert sh["n_ranks"] == 2 and sh["scaling"] == "strong" and sh["rays_per_s"] > 0
    assert res["eval_c5"]["f32"]["rays_per_s"] > 0


def _eval_setup(cfg, dev, rank, intrinsic=None):
    """eval.py:41-79 as codenerf.evaluate.eval_loop runs it: seeds, loaders, models, the optimiser's
    broadcast of rank 0's parameters (no checkpoint here), samplers and embedders."""
    from codenerf import nerf
    from codenerf.datasets import prepare_dataloader
    from codenerf.train import prepare_models, prepare_optimizer, seed_rank
    seed_rank(rank, cfg)
    loader, _ = prepare_dataloader("val", cfg, dev)
    _, train_dataset = prepare_dataloader("train", cfg, None)
    models = prepare_models(cfg, train_dataset.num_objects, dev)
    prepare_optimizer(cfg, models)
    first = next(iter(loader))
    (h, w), k = first["color"][0].shape[:2], first["intrinsic"][0]
    if intrinsic is not None:        # the single-process emulation: the ranks' samplers (eval.py:66-76)
        k = intrinsic
    samplers = nerf.prepare_samplers(cfg, h, w, k.cpu(), torch.float32, dev)
    return loader, models, samplers, nerf.prepare_embedders(cfg, torch.float32, dev), k.cpu()


def _eval_cfg(tree, logdir, world):
    from test_gpu_drivers import _cfg
    cfg = _cfg(tree, logdir, iterations=6, val_iterations=3)
    cfg.is_distributed, cfg.gpus = world > 1, world
    cfg.nerf.point_sampler.perturb = False     # a deterministic render to compare the gather bit for bit
    return cfg


def _eval_worker(rank, world, rdv, tree, out_dir):
    import numpy as np
    import torch.distributed as dist
    from codenerf.evaluate import validate
    dev = _init(rank, world, rdv)
    try:
        cfg = _eval_cfg(tree, os.path.join(out_dir, "e"), world)
        loader, models, samplers, embedders, k = _eval_setup(cfg, dev, rank)
        val = next(iter(loader))
        val = {"color": val["color"].clone(), "pose": val["pose"].clone()}
        if rank == 1:       # a different view on rank 1: validate must broadcast rank 0's (eval.py:111-115)
            val["color"] = val["color"].flip(1).contiguous()
        st = {"np": np.random.get_state(), "cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(dev)}
        res = validate(cfg, val, models, samplers, embedders, dev)
        out = {"np_keys": torch.from_numpy(st["np"][1].astype(np.int64)), "np_pos": st["np"][2],
               "np_hg": st["np"][3], "np_g": st["np"][4],
               "cpu_rng": st["cpu"], "cuda_rng": st["cuda"].cpu(), "zs": res["codes"][0].cpu(),
               "zt": res["codes"][1].cpu(), "cam_pose": res["cam_pose"].cpu(),
               "losses": torch.tensor([h["total_loss"] for h in res["history"]], dtype=torch.float64),
               "intrinsic": k}    # this rank's samplers' (its own first batch's, eval.py:66-76)
        if rank == 0:
            out.update(rgb=res["rgb"].cpu(), loss=res["loss"], psnr=res["psnr"], pose_error=res["pose_error"],
                       color=val["color"].cpu(), gt_pose=val["pose"].cpu(),
                       state={f"{k}.{n}": v.cpu() for k, m in models.items() for n, v in m.state_dict().items()})
        else:
            assert res["rgb"] is None and "loss" not in res
        torch.save(out, os.path.join(out_dir, f"eval{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_validate_two_ranks_q6(tmp_path):
    """eval.py:82-205 on two ranks (C5's multi-GPU eval): rank 0's view broadcast, every rank
    optimising codes and pose on its own ray draws (seed (r + 1) + randomseed), then
    parallel_image_render (nerf/__init__.py:137-226) with each rank rendering its Q5 slice from ITS OWN
    pose and codes (and, as eval.py:66-76 builds them, its own samplers from its own first validation
    batch).  Checked against a single process: (1) each rank's slice, rendered from that rank's
    optimised pose and codes, equals rank 0's gathered rows bit for bit; (2) re-running each rank's
    test_time_optimize from its recorded RNG state reproduces its losses, pose and codes bit for bit
    (the eval backward sums in a fixed order, cn_field_backward_fused_ws); (3) rank 0's loss / psnr /
    pose error are finite and the loss is the gathered image's MSE."""
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from srn_tree import write_tree
    from codenerf.evaluate import _pose_lr, test_time_optimize
    from codenerf.nerf import render_rays
    from codenerf.utils import split_sizes
    tree = write_tree(str(tmp_path / "srn"), channels=4)
    _spawn(_eval_worker, 2, tree, str(tmp_path))
    got = [torch.load(str(tmp_path / f"eval{r}.pt"), weights_only=True) for r in range(2)]
    dev = torch.device("cuda", 0)
    cfg = _eval_cfg(tree, str(tmp_path / "single"), 1)
    from codenerf import nerf
    _, models, _, emb, _ = _eval_setup(cfg, dev, 0)
    state = got[0]["state"]
    for k, m in models.items():
        m.load_state_dict({n[len(k) + 1:]: v for n, v in state.items() if n.startswith(k + ".")})
    color = got[0]["color"].to(dev, torch.float32)
    target = color.reshape(-1, color.shape[-1])
    gt_pose = got[0]["gt_pose"].to(dev, torch.float32)
    emb_t = models["embedding"]
    all_s, all_t = emb_t.get_all_embeddings(device=dev)
    e, o = cfg.experiment, cfg.optimizer
    rows = []
    per, _ = split_sizes(target.shape[0], 2)
    for r in range(2):
        g = got[r]
        h, w = got[0]["color"].shape[1:3]
        rs, ps = nerf.prepare_samplers(cfg, h, w, g["intrinsic"], torch.float32, dev)
        np.random.set_state(("MT19937", g["np_keys"].numpy().astype(np.uint32), int(g["np_pos"]), int(g["np_hg"]),
                             float(g["np_g"])))
        torch.set_rng_state(g["cpu_rng"])
        torch.cuda.set_rng_state(g["cuda_rng"], dev)
        zs, zt, _, hist, cam = test_time_optimize(target, (rs, ps), emb, models, (all_s.detach(), all_t.detach()),
                                                  e.val_iterations, val_lr=o.val_lr, angle_lr=_pose_lr(o, "angle_lr"),
                                                  radius_lr=_pose_lr(o, "radius_lr"),
                                                  regularizer_lambda=e.regularizer_lambda, gt_pose=gt_pose)
        assert torch.equal(torch.tensor([h["total_loss"] for h in hist], dtype=torch.float64), g["losses"]), r
        assert torch.equal(cam.cpu(), g["cam_pose"]), r
        assert torch.equal(zs.detach().cpu(), g["zs"]) and torch.equal(zt.detach().cpu(), g["zt"]), r
        # rank r's Q5 slice from its own optimised pose and codes, the validation chunking
        ro, rd = rs.get_bundle(tform_cam2world=g["cam_pose"].to(dev))
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        sl = slice(sum(per[:r]), sum(per[:r + 1]))
        n = ro.shape[0]
        with torch.no_grad():
            out = render_rays(ro[sl], rd[sl], g["zs"].to(dev).expand(n, -1)[sl], g["zt"].to(dev).expand(n, -1)[sl],
                              ps, emb, models["nerf_coarse"], models["nerf_fine"], cfg.nerf.validation.chunksize)
        rows.append(out["rgb_fine"].cpu())
    assert not torch.equal(got[0]["cam_pose"], got[1]["cam_pose"])      # the ranks optimised independently
    want = torch.cat(rows)
    assert torch.equal(got[0]["rgb"], want)
    assert np.isfinite([got[0]["loss"], got[0]["psnr"], got[0]["pose_error"]]).all()
    mse = ((got[0]["rgb"].double() - got[0]["color"].reshape(-1, 4)[:, :3].double()) ** 2).mean().item()
    assert abs(got[0]["loss"] - mse) <= 1e-6 * max(1.0, mse)


def _shard_worker(rank, world, rdv, tree, out_dir):
    import numpy as np
    import torch.distributed as dist
    from codenerf.evaluate import _pose_lr, sync_shard_state, test_time_optimize, validate
    dev = _init(rank, world, rdv)
    try:
        cfg = _eval_cfg(tree, os.path.join(out_dir, "s"), world)
        cfg.nerf.point_sampler.perturb = True        # the stratified / fine uniforms are sliced too
        loader, models, samplers, embedders, _ = _eval_setup(cfg, dev, rank)
        val = next(iter(loader))
        color = val["color"].to(dev, torch.float32).contiguous()
        gt_pose = val["pose"].to(dev, torch.float32).contiguous()
        dist.broadcast(color, 0)
        dist.broadcast(gt_pose, 0)
        sync_shard_state(samplers, 0)                 # rank 0's streams and camera on every rank
        st = {"np": np.random.get_state(), "cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(dev)}
        emb = models["embedding"]
        all_s, all_t = emb.get_all_embeddings(device=dev)
        e, o = cfg.experiment, cfg.optimizer
        zs, zt, pose, hist, cam = test_time_optimize(
            color.reshape(-1, color.shape[-1]), samplers, embedders, models, (all_s.detach(), all_t.detach()),
            e.val_iterations, val_lr=o.val_lr, angle_lr=_pose_lr(o, "angle_lr"), radius_lr=_pose_lr(o, "radius_lr"),
            regularizer_lambda=e.regularizer_lambda, gt_pose=gt_pose, shard_rays=True)
        out = {"np_keys": torch.from_numpy(st["np"][1].astype(np.int64)), "np_pos": st["np"][2],
               "np_hg": st["np"][3], "np_g": st["np"][4], "cpu_rng": st["cpu"], "cuda_rng": st["cuda"].cpu(),
               "zs": zs.detach().cpu(), "zt": zt.detach().cpu(), "cam_pose": cam.cpu(),
               "pose": torch.cat([v.detach().cpu() for v in pose]),
               "losses": torch.tensor([h["total_loss"] for h in hist], dtype=torch.float64),
               "intrinsic": samplers[0].intrinsics.cpu()}
        # end to end: validate's sharded mode (view broadcast, state sync, shared optimisation, gather)
        res = validate(cfg, {"color": val["color"], "pose": val["pose"]}, models, samplers, embedders, dev,
                       shard_rays=True)
        out.update(v_zs=res["codes"][0].cpu(), v_cam=res["cam_pose"].cpu())
        if rank == 0:
            out.update(color=color.cpu(), gt_pose=gt_pose.cpu(), v_loss=res["loss"], v_psnr=res["psnr"],
                       v_pose_error=res["pose_error"], v_rgb_rows=res["rgb"].shape[0],
                       state={f"{k}.{n}": v.cpu() for k, m in models.items() for n, v in m.state_dict().items()})
        torch.save(out, os.path.join(out_dir, f"shard{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_eval_ray_sharded_two_ranks(tmp_path):
    """The optional ray-sharded C5 mode (codenerf.evaluate.sharded_eval_step) on two
    ranks: ONE test-time optimisation whose every iteration's rays are split over the ranks (Q5 shares),
    the code / pose gradients summed by one all-reduce.  (1) Both ranks end with bit-identical codes and
    pose and the same loss history (they step on the same summed gradients).  (2) A single process that
    draws the same rays and uniforms (rank 0's recorded streams), renders the two shares one after the
    other, sums their gradients and steps reproduces every iteration's loss and the final pose and codes
    bit for bit (the eval backward sums in a fixed order; two ranks' all-reduce is one add).  (3) validate's
    sharded mode runs end to end: identical codes on both ranks, a finite loss / psnr / pose error and
    the whole gathered view on rank 0."""
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from srn_tree import write_tree
    from codenerf import nerf
    from codenerf.autograd import backward_from
    from codenerf.evaluate import _optimizer, _pose_lr, eval_step_loss, shard_draws, shard_of
    tree = write_tree(str(tmp_path / "srn"), channels=4)
    _spawn(_shard_worker, 2, tree, str(tmp_path))
    got = [torch.load(str(tmp_path / f"shard{r}.pt"), weights_only=True) for r in range(2)]
    for key in ("zs", "zt", "pose", "cam_pose", "losses", "v_zs", "v_cam"):
        assert torch.equal(got[0][key], got[1][key]), key
    # (2) the single-process emulation
    dev = torch.device("cuda", 0)
    cfg = _eval_cfg(tree, str(tmp_path / "single"), 1)
    cfg.nerf.point_sampler.perturb = True
    _, models, _, emb, _ = _eval_setup(cfg, dev, 0)
    g0 = got[0]
    for k, m in models.items():
        m.load_state_dict({n[len(k) + 1:]: v for n, v in g0["state"].items() if n.startswith(k + ".")})
        m.requires_grad_(False)
        m.train()
    color = g0["color"].to(dev)
    target = color.reshape(-1, color.shape[-1])
    gt_pose = g0["gt_pose"].to(dev)
    h, w = color.shape[1:3]
    rs, ps = nerf.prepare_samplers(cfg, h, w, g0["intrinsic"], torch.float32, dev)
    np.random.set_state(("MT19937", g0["np_keys"].numpy().astype(np.uint32), int(g0["np_pos"]), int(g0["np_hg"]),
                         float(g0["np_g"])))
    torch.set_rng_state(g0["cpu_rng"])
    torch.cuda.set_rng_state(g0["cuda_rng"], dev)
    all_s, all_t = models["embedding"].get_all_embeddings(device=dev)
    zs = all_s.detach().mean(dim=0, keepdim=True).clone().requires_grad_(True)
    zt = all_t.detach().mean(dim=0, keepdim=True).clone().requires_grad_(True)
    th, ph, rh = (torch.tensor([v], device=dev).requires_grad_(True) for v in (1.57, 0.0, 1.30))
    e, o = cfg.experiment, cfg.optimizer
    opt = _optimizer("AdamW", [{"params": [zs, zt]}, {"params": [th, ph], "lr": _pose_lr(o, "angle_lr")},
                               {"params": [rh], "lr": _pose_lr(o, "radius_lr")}], o.val_lr)
    params, n_rays, losses = [zs, zt, th, ph, rh], rs.sample_size, []
    for _ in range(e.val_iterations):
        sel, t_rand, u = shard_draws((rs, ps), n_rays)
        gsum, mse = None, None
        for r in range(2):
            sl = shard_of(n_rays, 2, r)
            loss, logs = eval_step_loss(th, ph, rh, zs, zt, target, (rs, ps), emb, models, e.regularizer_lambda,
                                        gt_pose=gt_pose, t_rand=t_rand[sl], u=u[sl], sel=sel[:, sl],
                                        rows_total=n_rays)
            opt.zero_grad()
            backward_from(loss)
            g = [p.grad.detach().clone() for p in params]
            m = torch.stack([logs["nerf_loss_coarse"], logs["nerf_loss_fine"]]) * ((sl.stop - sl.start) / n_rays)
            gsum = g if gsum is None else [a + b for a, b in zip(gsum, g)]
            mse = m if mse is None else mse + m
        with torch.no_grad():
            for p, g in zip(params, gsum):
                p.grad.copy_(g)
        opt.step()
        losses.append(float(mse[0] + mse[1] + logs["embedding_loss"]))
    assert losses[0] == g0["losses"][0].item()
    pose = torch.cat([v.detach().cpu() for v in (th, ph, rh)])
    assert losses == g0["losses"].tolist()
    for name, a, b in (("zs", zs.detach().cpu(), g0["zs"]), ("zt", zt.detach().cpu(), g0["zt"]),
                       ("pose", pose, g0["pose"])):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    # (3) validate's sharded mode
    assert np.isfinite([g0["v_loss"], g0["v_psnr"], g0["v_pose_error"]]).all()
    assert g0["v_rgb_rows"] == h * w


def _train_driver_worker(rank, world, rdv, tree, out_dir, tag, ckpt):
    import torch.distributed as dist
    from codenerf.train import train
    from test_gpu_drivers import _cfg
    dev = _init(rank, world, rdv)
    try:
        cfg = _cfg(tree, os.path.join(out_dir, tag), iterations=6, save_every=4, validate_every=1000)
        cfg.nerf.train.chunksize = 64                    # 128 rays per image -> 2 chunks per iteration
        cfg.is_distributed, cfg.gpus = True, world
        if ckpt:
            cfg = cfg | {"load_checkpoint": ckpt}
        out = train(rank, cfg, device=dev, verbose=False)
        torch.save({"params": {f"{k}.{n}": p.detach().cpu() for k, m in out["models"].items()
                               for n, p in m.named_parameters()},
                    "logs": torch.tensor([[lg[k] for k in sorted(lg)] for lg in out["logs"]], dtype=torch.float64),
                    "ckpts": list(out["checkpoints"])}, os.path.join(out_dir, f"{tag}{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_train_driver_two_ranks_mid_iteration_resume(tmp_path):
    """codenerf.train.train on 2 ranks: a save after chunk 0 of iteration 2 (i = 4; the
    driver gathers every rank's RNG streams into it with all_gather_object), then both ranks resume
    from it -- each restores its own streams and the cursor -- and must end with the uninterrupted
    2-rank run's parameters and chunk logs, bit for bit, on both ranks."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from srn_tree import write_tree
    tree = write_tree(str(tmp_path / "srn"), channels=4)
    _spawn(_train_driver_worker, 2, tree, str(tmp_path), "full", "")
    full = [torch.load(str(tmp_path / f"full{r}.pt"), weights_only=True) for r in range(2)]
    ck = [p for p in full[0]["ckpts"] if p.endswith("    4.ckpt")]
    assert ck, full[0]["ckpts"]
    _spawn(_train_driver_worker, 2, tree, str(tmp_path), "res", ck[0])
    res = [torch.load(str(tmp_path / f"res{r}.pt"), weights_only=True) for r in range(2)]
    n_after = res[0]["logs"].shape[0]
    assert n_after == full[0]["logs"].shape[0] - 5            # chunks 5.. of 12
    for r in range(2):
        assert torch.equal(res[r]["logs"], full[r]["logs"][5:]), r
        for k, v in full[r]["params"].items():
            assert torch.equal(res[r]["params"][k], v), (r, k)
    for k, v in full[0]["params"].items():
        assert torch.equal(full[1]["params"][k], v), ("ranks differ", k)
