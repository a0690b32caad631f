"""Shared by the ResNet LARS tests: flat-buffer tables ``[(length, adapted, planes, what)]`` that
break the tensor-aligned grid (CHUNK elements per workgroup), their inputs, and the comparison
against ``ops.layerwise.lars_mixed_update`` (float64)."""
import torch

import optim_reference as R
from distributedtensorflowexample_amd.ops import layerwise

CHUNK = 1024
TABLES = {
    # < 1 chunk; exactly 1; an excluded 1-D tensor between adapted ones; 1 chunk + 4; several with
    # a ragged last one; p = 0; g = 0; 2 and 3 planes (the second with padding behind the planes)
    "edges": [(512, True, 0, ""), (CHUNK, True, 0, ""), (64, False, 0, ""), (CHUNK + 4, True, 0, ""),
              (3 * CHUNK + 260, True, 0, ""), (CHUNK + 8, True, 0, "p0"), (256, True, 0, "g0"),
              (2 * CHUNK + 4, True, 2, ""), (1536, True, 3, "pad")],
    "twelve": [(64, False, 0, ""), (2 * CHUNK + 4, True, 0, ""), (64, False, 0, ""),  # > 8 tensors
               (64, False, 0, "g0"), (CHUNK, True, 2, ""), (4, True, 0, ""), (516, True, 0, ""),
               (64, False, 0, ""), (3 * CHUNK + 4, True, 0, ""), (8, False, 0, "p0"),
               (CHUNK + 4, True, 0, ""), (128, False, 0, "")],
}
# Roundings (half a float32 ulp each, of a magnitude <= the tensor's max |v|) behind one element of
# v per step: 6 in the element's own chain (gscale G, wd p, +, r *, mu v, +), 2 for a 3-plane sum,
# 5 in r (two square roots, fma, product, quotient) and, halved by the square root, the <= 24 of
# a sum of squares (4 per thread, 6 + 3 in the tree, twice: chunk and tensor): 6 + 2 + 5 + 12 = 25
# <= the 28 that bound(7) allows.  p adds its own two per step and lr (0.05) times v's error.
K_V, K_P = 7, 2
HYPER = dict(lr=0.05, momentum=0.9, eta=1.0)  # eta 1: g' is as large as g, r's error is visible


def make(table, seed, folds=True):
    """-> (tensors of the definition, LarsTable rows with CPU planes, p, g, v (f32), G (f64, planes
    summed): the gradient the rule sees; ``g`` holds 777 where planes cover a folded tensor)."""
    gen = torch.Generator().manual_seed(seed)
    n = sum(t[0] for t in table)
    p, g, v = torch.randn(n, generator=gen), torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen)
    G = g.double()
    tensors, rows, at = [], [], 0
    for length, adapted, S, what in table:
        if what == "p0":
            p[at:at + length] = 0
        if what == "g0":
            g[at:at + length] = 0
            G[at:at + length] = 0
        row = (at, length, adapted)
        if S and folds:
            plen = length - 36 if what == "pad" else length
            planes = torch.randn(S, plen + 8, generator=gen)  # (a stride longer than the planes)
            g[at:at + plen] = 777.0
            G[at:at + plen] = planes[:, :plen].double().sum(0)
            row += (planes, plen + 8, S, plen)
        tensors.append((at, length, adapted))
        rows.append(row)
        at += length
    return tensors, rows, p, g, v, G


def reference(p, G, v, tensors, wd, gscale):
    return layerwise.lars_mixed_update(p, G, v, R.f32(HYPER["lr"]), tensors, R.f32(HYPER["momentum"]),
                                       R.f32(wd), R.f32(HYPER["eta"]), R.f32(gscale))


def check(p, v, pb, ref_p, ref_v, tensors, steps, K_V=K_V):
    p, v = p.detach().cpu(), v.detach().cpu()
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())
    for k, (a, m, _) in enumerate(tensors):
        for name, out, ref, kk in (("p", p, ref_p, K_P), ("v", v, ref_v, K_V)):
            err = float((out[a:a + m].double() - ref[a:a + m]).abs().max())
            tol = R.bound(kk * steps, ref[a:a + m])
            assert err <= tol, "%s of tensor %d: max error %.3e > %.3e" % (name, k, err, tol)
    if pb is not None:
        assert torch.equal(pb.detach().cpu().view(torch.int16), p.to(torch.bfloat16).view(torch.int16))
