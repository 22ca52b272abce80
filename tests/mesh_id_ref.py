"""The checker of the collision-mesh object-id channel (sgs_render_mesh_ids*), built on the fp64 ray caster of tests/mesh_depth_ref.py.

The channel is this project's own definition (the reference has no such observation): a pixel's id is the label of the triangle whose hit
the depth frame reports — the least fp32 z among the hits with near < z <= far, the least label among hits at bit-equal z — and
ID_NONE where nothing is hit.  The kernel decides "hit" and z in fp32; this module says which labels a correct kernel may return, with
the depth reference's own bounds (eps_k per edge function, tol per depth: mesh_depth_ref's header derives them) and nothing more.

Admissible labels of a pixel.  Let `strict` be mesh_depth_ref.cast's value: the least z (1 + tol) over the triangles that claim the pixel
with margin (every edge function >= eps_k, z inside (near, far] by tol); +inf when there is none.  A kernel hits every such triangle and
computes a z of at most z (1 + tol) for it, so the z it keeps is <= strict; the triangle t it keeps passed the fp32 test, so it is a
lenient candidate (every edge function >= -eps_k, z inside (near, far] up to tol), and its exact z_t (1 - tol_t) is at most the fp32 z
the kernel computed for it.  Hence
    admissible = { label(t) : t a lenient candidate with z_t (1 - tol_t) <= strict },
and ID_NONE is admissible exactly when strict == +inf (no triangle has to be hit).  The pass rule is  got in admissible.
A pixel is DECIDED when its set has one element: there the rule is an equality.  Away from silhouettes and from the contact lines of
objects every pixel is decided; `check` returns the decided share so that a test can demand it (a checker that leaves everything
undecided would pass anything).
"""
from __future__ import annotations

import numpy as np

import mesh_depth_ref as ref

ID_NONE = -1


def admissible(vertices, triangles, labels, cam, near=0.2, far=1.0e30, pixels=None, chunk=1 << 21):
    """dict(shape, strict, labels (sorted distinct labels), member bool [P, L]: label l is admissible at pixel p, none_ok bool [P],
    count [P] = size of the set, decided bool [P], value int64 [P] = the set's element where decided).  ref: the depth reference of the
    same frame (mesh_depth_ref.cast), for checking the depth that comes with the ids."""
    W, H = cam["width"], cam["height"]
    if pixels is None:
        ys, xs = np.divmod(np.arange(W * H), W)
        shape = (H, W)
    else:
        ys, xs = (np.asarray(a, np.int64) for a in pixels)
        shape = (len(ys),)
    T = np.asarray(triangles).reshape(-1, 3)
    lab = np.asarray(labels, np.int64).reshape(-1)
    assert len(lab) == len(T) and (lab >= 0).all()
    depth = ref.cast(vertices, T, cam, near=near, far=far, pixels=pixels, chunk=chunk)
    strict = depth["strict"].reshape(-1)
    uniq = np.unique(lab)
    member = np.zeros((len(ys), len(uniq)), bool)
    if len(T) and len(ys):
        for pix, t, s, eps, z, tol in ref._candidates(vertices, T, cam, near, xs, ys, chunk):
            ok = np.isfinite(z)
            lin = (s >= -eps).all(1) & ok & (z * (1 + tol) > near) & (z * (1 - tol) <= far)
            adm = lin & (z * (1 - tol) <= strict[pix])
            member[pix[adm], np.searchsorted(uniq, lab[t[adm]])] = True
    none_ok = np.isinf(strict)
    count = member.sum(1) + none_ok
    decided = count == 1
    value = np.where(none_ok, ID_NONE, uniq[member.argmax(1)] if len(uniq) else ID_NONE)
    return dict(shape=shape, strict=strict, labels=uniq, member=member, none_ok=none_ok, count=count, decided=decided,
                value=np.where(decided, value, ID_NONE - 1), ref=depth)


def passes(got, adm):
    """bool [P]: got is in the pixel's admissible set."""
    got = np.asarray(got, np.int64).reshape(-1)
    uniq, member = adm["labels"], adm["member"]
    k = np.clip(np.searchsorted(uniq, got), 0, max(len(uniq) - 1, 0))
    known = (uniq[k] == got) if len(uniq) else np.zeros(len(got), bool)
    in_set = known & member[np.arange(len(got)), k] if len(uniq) else known
    return np.where(got == ID_NONE, adm["none_ok"], in_set)


def check(got, adm, what=""):
    """The pass rule on every pixel; prints the counts.  Returns (decided share, distinct labels among the decided pixels)."""
    got = np.asarray(got).reshape(-1)
    assert got.size == adm["count"].size, (got.size, adm["count"].size)
    ok = passes(got, adm)
    dec = adm["decided"]
    share = float(dec.mean()) if dec.size else 1.0
    dl = np.unique(adm["value"][dec & (adm["value"] >= 0)])
    print(f"mesh ids {what}: {got.size} px, decided {int(dec.sum())} ({100 * share:.1f} %), {len(dl)} decided labels, "
          f"failing {int((~ok).sum())}, none {int((got == ID_NONE).sum())}")
    if not ok.all():
        i = np.flatnonzero(~ok)[:8]
        sets = [adm["labels"][adm["member"][j]].tolist() + ([ID_NONE] if adm["none_ok"][j] else []) for j in i]
        raise AssertionError(f"{what}: {int((~ok).sum())} pixels with an id outside the admissible set ({int((~ok & dec).sum())} of them "
                             f"decided); first {i.tolist()}: got {got[i].tolist()} admissible {sets}")
    return share, len(dl)
