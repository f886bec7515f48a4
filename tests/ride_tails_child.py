"""Child process of tests/test_gpu_ride_tails.py: runs the scenarios once under whatever PNPP_RIDE_TAILS the parent set (the switch is
read once per process) and leaves the gradients (result.pt) and the launch tags (tags.json) in the directory given.

    python tests/ride_tails_child.py OUTDIR

Levels (the smallest at which both launches of a pair exist -- see the parent's docstring):
    lower      grouped    B 2, N 128, S 64, K 16, D 32, mlp [32, 32, 64]    (G = 128 groups: opens its backward with pool_bwd_kernel)
    upper_all  group_all  B 2, N 64,        D 64, mlp [64, 64, 128]         (128 rows: layer 0's dW in 4 partials)
    upper_grp  grouped    B 2, N 64, S 8, K 8, D 64, mlp [64, 64, 128]      (128 rows: the same)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-pointcloud-orientation-estimation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dispatch import record  # noqa: E402
from models.pointnet_pp_8dir import PointNetSetAbstraction  # noqa: E402
from pnpp_hip import ops  # noqa: E402
from pnpp_hip.optim import FlatAdam  # noqa: E402

DEV = torch.device("cuda")
B, N, S, K, D = 2, 128, 64, 16, 32


class Pair:
    """lower -> upper on fixed inputs and injected centres; every parameter gradient goes to one FlatAdam buffer."""

    def __init__(self, upper: str, lower: bool = True, train_lower: bool = True, seed: int = 0):
        g = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        self.lower = PointNetSetAbstraction(S, K, D, [32, 32, 64]).to(DEV).train() if lower else None
        if upper == "all":
            self.upper = PointNetSetAbstraction(None, None, 64, [64, 64, 128], group_all=True).to(DEV).train()
            self.c2 = None
        else:
            self.upper = PointNetSetAbstraction(8, 8, 64, [64, 64, 128]).to(DEV).train()
            self.c2 = torch.stack([torch.randperm(S, generator=g)[:8] for _ in range(B)]).to(DEV)
        self.xyz = torch.rand(B, N, 3, generator=g).to(DEV)
        self.c1 = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)]).to(DEV)
        self.weight = torch.randn(B, 1, 128, generator=g).to(DEV)
        params = list(self.upper.parameters())
        if lower:
            self.feats = torch.randn(B, N, D, generator=g).to(DEV).requires_grad_(train_lower)
            if train_lower:
                params = list(self.lower.parameters()) + params
            else:
                for p in self.lower.parameters():
                    p.requires_grad_(False)
        else:   # the upper level alone, on a leaf that wants its gradient
            self.feats = torch.randn(B, S, 64, generator=g).to(DEV).requires_grad_(True)
            self.xyz = self.xyz[:, :S].contiguous()
        self.opt = FlatAdam(params, fused_grads=True)

    def step(self):
        self.opt.zero_grad()
        xyz, pts = self.xyz, self.feats
        if self.lower is not None:
            xyz, pts = self.lower(xyz, pts, centre_idx=self.c1)
        _, out = self.upper(xyz, pts, centre_idx=self.c2)
        (out * self.weight).sum().backward()

    def grads(self):
        g = {"flat": self.opt.flat_g.detach().cpu().clone()}
        if self.feats.grad is not None:
            g["input"] = self.feats.grad.detach().cpu().clone()
        return g


def main(out_dir):
    res, tags = {}, {}

    def run(name, pair):
        tags[name] = record(pair.step)
        res[name] = pair.grads()
        res[name]["pending_after"] = ops.pending_tails()

    run("pair_all", Pair("all"))
    run("pair_grp", Pair("grp"))
    run("frozen_all", Pair("all", train_lower=False))
    run("alone_all", Pair("all", lower=False))
    run("alone_grp", Pair("grp", lower=False))

    # two passes in a row, then one captured pass replayed twice: the same gradients every time, nothing left pending
    p = Pair("all")
    passes = []
    for _ in range(2):
        p.feats.grad = None
        p.step()
        passes.append((p.grads(), ops.pending_tails()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the capture stream's own workspaces exist before the capture
        p.feats.grad = None
        p.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    p.feats.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        p.step()
    captured_pending = ops.pending_tails()
    for _ in range(2):
        p.opt.flat_g.fill_(float("nan"))   # a replay that left a reduction out would leave this behind
        graph.replay()
        torch.cuda.synchronize()
        passes.append((p.grads(), captured_pending))
    res["passes"] = [g for g, _ in passes]
    res["passes_pending"] = [n for _, n in passes]

    torch.save(res, os.path.join(out_dir, "result.pt"))
    with open(os.path.join(out_dir, "tags.json"), "w") as f:
        json.dump(tags, f, indent=1)
    print("ride_tails_child: done")


if __name__ == "__main__":
    main(sys.argv[1])
