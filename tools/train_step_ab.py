"""cfg-2 train.py step (bench.train_step_bench) on the live-region regulariser under autograd
(default) or forward_full (--full: MVS_TRAIN_LIVE=0), under an assignment of the training switches
(--switches: a preset of mvs_amd/train_switches.py, "default" or "all_hip", or NAME=value,NAME=value; printed
in the JSON line as "switches"), with a per-kernel summary from the torch profiler of one step (--prof).

--loss package runs the step with mvs_amd.loss.loss_fcn (csrc/loss.hip) in the place of bench.py's torch expression
(printed as "loss_fcn"); with --prof the objective's own forward + backward is profiled once more on its own and its
kernel launches and device time printed as one JSON line.

Usage: python tools/train_step_ab.py [--switches all_hip] [--full] [--steps N] [--prof] [--loss torch|package]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--ops", action="store_true", help="with --prof: aten ops grouped by input shape")
    ap.add_argument("--switches", default="default", metavar="PRESET_OR_ASSIGNMENTS",
                    help="a preset of mvs_amd/train_switches.py (default, all_hip) or NAME=value,NAME=value")
    ap.add_argument("--loss", choices=("torch", "package"), default="torch",
                    help="the objective of the step: bench.py's torch expression (default: the numbers on record) "
                         "or mvs_amd.loss.loss_fcn (the HIP kernels of csrc/loss.hip)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "deep-multiview-depth-estimation_amd"))
    from mvs_amd import train_switches
    assignment = train_switches.parse_assignment(a.switches)
    if a.full:
        assignment["MVS_TRAIN_LIVE"] = "0"
    os.environ.update(assignment)   # before bench is imported
    import bench
    import torch
    if a.loss == "package":   # bench.train_step_bench and the profiled step below look the objective up in bench
        from mvs_amd.loss import loss_fcn
        bench.masked_mae_loss = lambda gt, initial, refined: loss_fcn(gt, initial, refined)[0]
    dev = torch.device("cuda", 0)
    out = bench.train_step_bench(4, 3, 192, 512, 640, dev, a.steps)
    out["switches"] = assignment
    out["loss_fcn"] = a.loss
    print(json.dumps(out), flush=True)
    if a.prof:
        from torch.profiler import ProfilerActivity, profile
        net = bench.build_model(192, 512, 640, dev).train()
        opt = torch.optim.Adam(net.parameters, lr=1e-3)
        img, K, R, T, d_min, d_int = bench.make_inputs(4, 3, 512, 640, 0, dev)
        gt = (425.0 + 25.0 * 192 * torch.rand(4, 1, 128, 160)).to(dev)

        def step():
            opt.zero_grad(set_to_none=True)
            ini, ref = net(img, K, R, T, d_min, d_int, 4, 3)
            bench.masked_mae_loss(gt, ini, ref).backward()
            opt.step()
        step()
        torch.cuda.synchronize()
        acts = [ProfilerActivity.CUDA] + ([ProfilerActivity.CPU] if a.ops else [])
        with profile(activities=acts, record_shapes=a.ops) as p:
            step()
            torch.cuda.synchronize()
        print(p.key_averages().table(sort_by="cuda_time_total", row_limit=30, max_name_column_width=70), flush=True)
        if a.ops:
            print(p.key_averages(group_by_input_shape=True).table(sort_by="self_cuda_time_total", row_limit=45,
                                                                  max_name_column_width=40,
                                                                  max_shapes_column_width=110), flush=True)
        # the objective alone, forward + backward on the step's own maps: its launches and device time
        with torch.no_grad():
            ini, ref = (t.detach().clone().requires_grad_(True) for t in net(img, K, R, T, d_min, d_int, 4, 3))
        bench.masked_mae_loss(gt, ini, ref).backward()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as p:
            bench.masked_mae_loss(gt, ini, ref).backward()
            torch.cuda.synchronize()
        rows = [r for r in p.key_averages() if r.self_device_time_total > 0]   # kernels, not the runtime's calls
        print(json.dumps({"loss_fcn": a.loss, "loss_fwd_bwd_launches": sum(r.count for r in rows),
                          "loss_fwd_bwd_device_us": sum(r.device_time_total for r in rows)}), flush=True)
        print(p.key_averages().table(sort_by="cuda_time_total", row_limit=40, max_name_column_width=90), flush=True)


if __name__ == "__main__":
    main()
