#!/usr/bin/env python3
"""oracle/make_index_edges.py -- TEST INFRASTRUCTURE ONLY.

tests/golden/index_edges.npz: the edges of the index primitives, captured from the reference itself (imported read-only, as
oracle/make_golden.py does; no reference source is copied).  Every expected output is what the reference's own function object
returned; nothing here comes from oracle/ or from the HIP kernels.  Writes that one file and touches no other fixture.

    python oracle/make_index_edges.py [out.npz]

Radius boundary, per radius r in RADII (tag rb_<r>), t = float32(r ** 2), the value PointNet++Demo.py:65 compares against:
    rb_<r>_xyz         (1,M,3) float32   a shuffled cloud: candidates whose squared distance to the centre -- by the reference's own
                                         expression (:63), in float32 -- is exactly t - 1 ulp, t, t + 1 ulp, t + 2 ulp (several of each,
                                         found by a seeded 3-D search), points clearly inside and clearly outside, and the centre
    rb_<r>_new_xyz     (1,1,3) float32   the centre (off the origin, so the differences round); it is row rb_<r>_centre_idx of the cloud
    rb_<r>_bits        (M,)    uint32    the bit pattern of every point's squared distance
    rb_<r>_idx         (1,1,M) int16     demo.query_ball_point(r, M, xyz, new_xyz): nothing is cut off
    rb_<r>_idx_cut     (1,1,CUT) int16   the same call with nsample = CUT: the first CUT members in ascending index order; the cloud's
                                         first HEAD rows hold more than CUT clearly-inside points and no boundary candidate
    rb_radii (R,) float64, rb_t_bits (R,) uint32 (torch's own float32 of r ** 2)
Other edges: be_* (radius query: empty, under-full, nsample == N), fd_* / fo_* / f1_* (Demo FPS: duplicated points, npoint > N, N = 1;
start indices replayed as golden_index() does), sqself_* (square_distance of a cloud with coincident points against itself, as bits),
kq_* (base.query_ball_point = kNN on a tie-free cloud, k == N and k == 1, as sorted sets).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_demo, n  # noqa: E402  (puts the reference on sys.path: `models` below is the reference's package)
from make_tail_golden import npz_bytes  # noqa: E402

DEFAULT = os.path.join(HERE, "..", "tests", "golden", "index_edges.npz")
RADII = (0.05, 0.1, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.8)
PER_TARGET, HEAD, CUT = 4, 6, 3
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def ref_sqrdists(new_xyz, xyz):
    """the reference's own expression (PointNet++Demo.py:63) on float32 tensors -> (S,N) numpy"""
    new_xyz, xyz = torch.from_numpy(new_xyz)[None], torch.from_numpy(xyz)[None]
    return torch.sum((new_xyz.unsqueeze(2) - xyz.unsqueeze(1)) ** 2, -1)[0].numpy()


def hunt(r, centre, rng):
    """Points whose squared distance to `centre` is exactly one of the four targets around t = float32(r ** 2): a random direction,
    scaled to the radius, then one coordinate stepped with nextafter towards t; the walk crosses t back and forth and lands on the
    float32 values next to it.  -> {target bits: (PER_TARGET,3) float32}"""
    t = F32(r ** 2)
    targets = [int(bits(t)[0]) + k for k in (-1, 0, 1, 2)]        # positive float32: neighbouring values are neighbouring bit patterns
    found = {tb: [] for tb in targets}
    for _ in range(200):
        M = 2048
        u = rng.standard_normal((M, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        p = (centre.astype(np.float64) + u * r).astype(F32)
        axis = rng.integers(0, 3, M)
        rows = np.arange(M)
        for _step in range(48):
            d = ref_sqrdists(centre[None], p)[0]
            db = bits(d)
            for tb in targets:
                for i in np.flatnonzero(db == tb):
                    if len(found[tb]) < PER_TARGET and not any(np.array_equal(p[i], q) for q in found[tb]):
                        found[tb].append(p[i].copy())
            if all(len(v) >= PER_TARGET for v in found.values()):
                return {tb: np.stack(v) for tb, v in found.items()}
            outward = np.where(p[rows, axis] >= centre[axis], F32(np.inf), F32(-np.inf)).astype(F32)
            toward = np.where(d < t, outward, -outward).astype(F32)
            p[rows, axis] = np.nextafter(p[rows, axis], toward, dtype=F32)
    raise AssertionError(f"radius {r}: targets not all hit: { {hex(k): len(v) for k, v in found.items()} }")


def radius_boundary(demo, out):
    t_bits = []
    for ri, r in enumerate(RADII):
        rng = np.random.default_rng(20261021 + ri)
        t = F32(r ** 2)
        tt = torch.tensor(r ** 2, dtype=torch.float32).numpy()             # torch's own rounding of the python scalar
        assert bits(tt) == bits(t)
        t_bits.append(int(bits(t)[0]))
        centre = (rng.uniform(0.3, 0.9, 3) * rng.choice([-1.0, 1.0], 3)).astype(F32)
        hits = hunt(r, centre, rng)

        def shell(lo, hi, m):
            u = rng.standard_normal((m, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            return (centre.astype(np.float64) + u * (r * rng.uniform(lo, hi, (m, 1)))).astype(F32)

        inside, outside = shell(0.2, 0.9, HEAD - 2 + 3), shell(1.1, 2.0, 2 + 3)
        head = np.concatenate([inside[:HEAD - 2], outside[:2]])             # HEAD rows: more than CUT members, no boundary candidate
        rest = np.concatenate([inside[HEAD - 2:], outside[2:], centre[None]] + list(hits.values()))
        xyz = np.concatenate([head[rng.permutation(len(head))], rest[rng.permutation(len(rest))]])[None]
        new_xyz = centre[None, None]
        M = xyz.shape[1]
        centre_idx = int(np.flatnonzero((xyz[0] == centre).all(1))[0])
        db = bits(ref_sqrdists(new_xyz[0], xyz[0])[0])
        for tb in hits:                                                     # all four targets are in the cloud that is stored
            assert (db == tb).sum() >= PER_TARGET, (r, hex(tb))
        assert not np.isin(db[:HEAD], list(hits)).any()
        full = n(demo.query_ball_point(r, M, torch.from_numpy(xyz), torch.from_numpy(new_xyz)))
        cut = n(demo.query_ball_point(r, CUT, torch.from_numpy(xyz), torch.from_numpy(new_xyz)))
        members = set(full[0, 0].tolist())
        assert M not in members and centre_idx in members
        at = lambda k: np.flatnonzero(db == t_bits[-1] + k)                 # the reference's rule, read off its own list
        assert all(i in members for i in np.concatenate([at(-1), at(0)])) and not any(i in members for i in np.concatenate([at(1), at(2)]))
        assert len(members) > CUT and len(set(range(HEAD)) & members) > CUT and cut.max() < HEAD
        tag = f"rb_{r}"
        out.update({f"{tag}_xyz": xyz, f"{tag}_new_xyz": new_xyz, f"{tag}_bits": db, f"{tag}_idx": full.astype(np.int16),
                    f"{tag}_idx_cut": cut.astype(np.int16), f"{tag}_centre_idx": np.array(centre_idx, np.int32)})
        print(f"r={r}: t={hex(t_bits[-1])} M={M} members={len(members)} "
              f"at t: {sorted(i in members for i in np.flatnonzero(db == t_bits[-1]))} "
              f"at t+1ulp: {sorted(i in members for i in np.flatnonzero(db == t_bits[-1] + 1))}")
    out["rb_radii"] = np.array(RADII, np.float64)
    out["rb_t_bits"] = np.array(t_bits, np.uint32)


def ball_edges(demo, out):
    g = torch.Generator().manual_seed(20261022)
    # empty: nothing within the radius of any centre -> every slot is N
    xyz = torch.rand(2, 20, 3, generator=g)
    new = torch.full((2, 3, 3), 50.0) + torch.rand(2, 3, 3, generator=g)
    idx = demo.query_ball_point(0.2, 5, xyz, new)
    assert bool((idx == 20).all())
    out.update(be_empty_xyz=n(xyz), be_empty_new_xyz=n(new), be_empty_idx=n(idx).astype(np.int16))
    # under-full: fewer members than nsample -> padded with the first member (and one empty row among them)
    xyz = torch.rand(2, 64, 3, generator=g)
    new = torch.cat([xyz[:, 5:12], torch.full((2, 1, 3), -7.0)], 1).contiguous()
    idx = demo.query_ball_point(0.25, 16, xyz, new)
    rows = n(idx).reshape(-1, 16)
    distinct = [len(set(row.tolist())) for row in rows]
    assert sum(1 < d < 16 for d in distinct) >= 4 and any(row[0] == 64 for row in rows)
    assert all((row[d:] == row[0]).all() for row, d in zip(rows, distinct))
    out.update(be_under_xyz=n(xyz), be_under_new_xyz=n(new), be_under_idx=n(idx).astype(np.int16))
    # nsample == N and everything inside -> arange(N)
    xyz = torch.rand(2, 33, 3, generator=g) * 0.2
    new = torch.rand(2, 4, 3, generator=g) * 0.2
    idx = demo.query_ball_point(1.0, 33, xyz, new)
    assert torch.equal(idx, torch.arange(33).expand(2, 4, 33))
    out.update(be_full_xyz=n(xyz), be_full_new_xyz=n(new), be_full_idx=n(idx).astype(np.int16))


def fps_edges(demo, out):
    g = torch.Generator().manual_seed(20261023)

    def capture(tag, xyz, npoint, seed):
        B, N, _ = xyz.shape
        torch.manual_seed(seed)
        fps = demo.farthest_point_sample(xyz, npoint)
        torch.manual_seed(seed)                                             # replay the randint draw (:20)
        start = torch.randint(0, N, (B,), dtype=torch.long)
        assert torch.equal(fps[:, 0], start)
        out.update({f"{tag}_xyz": n(xyz), f"{tag}_start": n(start).astype(np.int32), f"{tag}_idx": n(fps).astype(np.int16)})
        return fps

    base = torch.rand(2, 300, 3, generator=g)                               # duplicated points: exact ties, first maximum wins
    xyz = torch.cat([base, base, base[:, :100]], 1)
    xyz = torch.stack([xyz[b, torch.randperm(700, generator=g)] for b in range(2)])
    assert len({p.tobytes() for p in n(xyz[0])}) == 300
    capture("fd", xyz, 64, 11)
    fps = capture("fo", torch.rand(2, 10, 3, generator=g), 25, 12)          # npoint > N: points are revisited
    assert all(len(set(row.tolist())) == 10 for row in fps)
    fps = capture("f1", torch.rand(3, 1, 3, generator=g), 4, 13)            # N = 1
    assert bool((fps == 0).all())


def base_edges(out):
    from models import base
    g = torch.Generator().manual_seed(20261024)
    pts = torch.rand(2, 25, 3, generator=g) * 4 - 2                         # coincident points: sampled with replacement
    xyz = torch.stack([pts[b, torch.randint(0, 25, (40,), generator=g)] for b in range(2)])
    d = n(base.square_distance(xyz, xyz))
    diag = d[:, np.arange(40), np.arange(40)]
    assert (diag != 0).any() and (diag < 0).any(), "the diagonal is expected to carry rounding residue"
    out.update(sqself_xyz=n(xyz), sqself_bits=bits(d))
    xyz = torch.rand(2, 33, 3, generator=g) * 2 - 1                         # kNN, k == N and k == 1, tie-free
    new = torch.cat([xyz[:, 3:7], torch.rand(2, 3, 3, generator=g) * 2 - 1], 1).contiguous()
    dist = n(base.square_distance(new, xyz))
    assert all(len(np.unique(row)) == 33 for row in dist.reshape(-1, 33))
    all_k = n(base.query_ball_point(new, xyz, 33))
    one_k = n(base.query_ball_point(new, xyz, 1))
    assert (np.sort(all_k, -1) == np.arange(33)).all() and (one_k[:, :4, 0] == np.arange(3, 7)).all()
    out.update(kq_xyz=n(xyz), kq_new_xyz=n(new), kq_idx33_sorted=np.sort(all_k, -1).astype(np.int16),
               kq_idx1_sorted=np.sort(one_k, -1).astype(np.int16))


def main(argv):
    torch.set_num_threads(8)
    demo = load_demo()
    out = {}
    radius_boundary(demo, out)
    ball_edges(demo, out)
    fps_edges(demo, out)
    base_edges(out)
    path = argv[1] if len(argv) > 1 else DEFAULT
    data = npz_bytes(out)
    with open(path, "wb") as f:
        f.write(data)
    print(f"wrote {os.path.normpath(path)}: {len(data) / 1024:.1f} KiB")


if __name__ == "__main__":
    main(sys.argv)
