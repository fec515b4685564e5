"""Writes tests/golden/reference_seams.npz: what the reference's own compiled
kernel bodies (oracle/_ref/libo3d_ref.so through tests/_ref.py) return on the
inputs of tests/_seam_cases.py. Data only; every array is reproduced byte for
byte by running this again (tests/test_seams_vs_ref.py checks that).

    fpfh/<fixture>/<dtype>/lists   ComputeFPFHFeatureCPU rows (padded == CSR)
    fpfh/<fixture>/<dtype>/mask    the rows of the filtered form
    doppler/vs/<n>/<dtype>         PreComputeForDopplerICPKernelCPU
    doppler/<case>/exact|mag|count exactly rounded column sums of the per-pair
                                   29 terms, sum |terms|, pairs
    doppler/<case>/digest          SHA-256 of the per-pair terms {n, 29}
    doppler/<case>/terms           the per-pair terms themselves (n <= 65, L2)
    rigid/<case>/exact|mag|digest  the same for the pairs' 12x12 + 12 + 1, and
                                   `whole`: the whole-set 12x12 block, rhs,
                                   residual (one thread)
    alignment/<case>/digest        SHA-256 of the pairs' 60x60 products, 60
                                   rhs products and r^2 (distinct node labels)
    alignment/<case>/whole_digest, whole_b, whole_r
                                   the whole-set system (one thread)
    regularizer/<case>/at|values|b|r
                                   the non-zero AtA entries, Atb, residual

A 1025-pair case holds 3.7 million products: the record keeps their digest,
and the GPU test recomputes them with the restatement, checks the digest and
only then sums them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _ref as ref  # noqa: E402
import _seam_cases as sc  # noqa: E402
import _slac_nonrigid_oracle as no  # noqa: E402

F = np.float32


def build():
    ref.set_threads(1)
    out = {}
    for fixture in ("generic", "lattice"):
        for dt in sc.DTYPES:
            case = sc.fpfh_case(fixture, dt)
            for form, key in (("padded", "lists"), ("mask", "mask")):
                lists, rows, mask = sc.fpfh_form(case, form)
                out["fpfh/%s/%s/%s" % (fixture, np.dtype(dt).name, key)] = \
                    ref.fpfh_from_lists(case["points"], case["normals"],
                                        **lists, list_points=rows, mask=mask)
    for dt in sc.DTYPES:
        for n in sc.DOPPLER_SIZES:
            case = sc.doppler_case(n, np.dtype(dt).name)
            out["doppler/vs/%d/%s" % (n, np.dtype(dt).name)] = \
                ref.doppler_precompute(*case["prep"])
    for s in sc.doppler_settings():
        case = sc.doppler_case(s["n"], s["dtype"])
        terms = ref.doppler_pair_terms(
            *case["arrays"], *case["prep"], sc.PERIOD, s["reject"],
            sc.DOPPLER_THRESHOLD, s["kg"], s["kd"], s["lam"])
        exact, mag = sc.exact_columns(terms)
        key = "doppler/%s/" % s["name"]
        out[key + "exact"], out[key + "mag"] = exact, mag
        out[key + "count"] = np.array(int((case["arrays"][5] != -1).sum()))
        out[key + "digest"] = sc.digest(terms)
        if s["n"] <= 65 and s["name"].startswith("l2"):
            out[key + "terms"] = terms
    for name in sc.SLAC_CASES:
        arrays, thr = sc.slac_case(name)
        p, q, n, _ = sc.rigid_inputs(name)
        A, b, r2 = ref.fill_in_rigid_alignment_pairs(p, q, n, thr)
        flat = np.concatenate([A.reshape(len(A), -1), b, r2[:, None]], 1)
        key = "rigid/%s/" % name
        out[key + "exact"], out[key + "mag"] = sc.exact_columns(flat)
        out[key + "digest"] = sc.digest(A, b, r2)
        z = (np.zeros((18, 18), F), np.zeros(18, F), np.zeros(1, F))
        wA, wb, wr = ref.fill_in_rigid_alignment_term(*z, p, q, n, *sc.EDGE,
                                                      thr)
        out[key + "whole"] = np.concatenate([wA[6:, 6:].reshape(-1), wb[6:],
                                             wr])
        A, b, r2 = ref.fill_in_slac_alignment_pairs(sc.relabelled(arrays), 0,
                                                    1, 2, thr, 60)
        key = "alignment/%s/" % name
        out[key + "digest"] = sc.digest(A, b, r2)
        z = (np.zeros((sc.N_VARS, sc.N_VARS), F), np.zeros(sc.N_VARS, F),
             np.zeros(1, F))
        wA, wb, wr = ref.fill_in_slac_alignment_term(*z, arrays, *sc.EDGE,
                                                     sc.N_FRAGS, thr)
        out[key + "whole_digest"] = sc.digest(wA)
        out[key + "whole_b"], out[key + "whole_r"] = wb, wr
    for name, g, curr, masks in no.regularizer_cases():
        want = ref.fill_in_slac_regularizer_term(
            np.arange(64), g.nbs_idx, masks, g.init, curr, sc.REG_WEIGHT,
            sc.N_FRAGS, g.anchor, sc.N_VARS)
        at = np.flatnonzero(want["AtA"]).astype(np.int32)
        key = "regularizer/%s/" % name
        out[key + "at"] = at
        out[key + "values"] = want["AtA"].reshape(-1)[at]
        out[key + "b"] = want["Atb"]
        out[key + "r"] = np.array(want["residual"], np.float32)
    return out


if __name__ == "__main__":
    arrays = build()
    path = os.path.join(HERE, "reference_seams.npz")
    np.savez(path, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (path, len(arrays),
                                             os.path.getsize(path)))
