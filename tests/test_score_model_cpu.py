"""The float64 model of predict() that test_score_fp64_gpu.py holds the scorers against (tests/score_model.py), checked on its own:
it reproduces the reference's recorded predict() of every golden fixture, its float32 evaluation passes the shared tolerance rule
on every input family, and ten value mutants of it -- the mistakes a scorer kernel could make without faulting -- each fail the
rule on the case meant to catch them. No GPU."""
import numpy as np
import pytest
import torch

import score_model as sm
from helpers import load_golden, sub

FIXTURES = ["ml3", "kwai", "ablate", "gcmc", "normal", "tiktok"]


def _fixture_table(g):
    """Y, U, d, S, head_mask of a fixture's cached tables, laid out as the scorers get them (Kwai has the single head v; the mask
    names the heads of --modality, models/EliMRec.py:133-134, 171-184)."""
    c = sub(g, "cache")
    mods = ["v"] if str(g["dataset_name"]) == "kwai" else ["v", "a", "t"]
    users = [c["all_users"]] + [c["pre_fusion_user_" + m] for m in mods]
    items = [c["all_items"]] + [c["pre_fusion_item_" + m] for m in mods]
    Y = torch.from_numpy(np.concatenate([np.concatenate(users, 1), np.concatenate(items, 1)], 0))
    mask = sum(1 << h for h, m in enumerate(mods) if m in str(g["modality"]))
    return Y, c["all_users"].shape[0], c["all_users"].shape[1], len(mods), mask


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reproduces_the_references_recorded_predict(name):
    """float64 model on the cached tables against the float32 predict() the reference recorded, every fusion mode and predict
    type: within the shared rule (4 x the float32 model's own distance from float64, at least 2.4e-7)."""
    g = load_golden(name)
    Y, U, d, S, mask = _fixture_table(g)
    assert U == int(g["num_users"]) and d == int(g["recdim"])
    users = torch.from_numpy(g["eval_users"].astype(np.int64))
    recorded = sub(g, "predict")
    assert len(recorded) == 7
    for key, want in recorded.items():
        fusion, ptype = key.split("/")
        ref64 = sm.score_model(Y.double(), U, users, d, S, mask, fusion, ptype)
        ref32 = sm.score_model(Y, U, users, d, S, mask, fusion, ptype)
        tol, e32 = sm.tolerance(ref64, ref32, fast=False)
        err = sm.worst_error(torch.from_numpy(want), ref64)
        assert err <= tol, (name, key, err, tol, e32)
    if name in ("ablate", "gcmc"):          # the mask matters there: rubi with every head is another function
        full = sm.score_model(Y.double(), U, users, d, S, 0b111, "rubi", "TE")
        assert sm.worst_error(torch.from_numpy(recorded["rubi/TE"]), full) > 1e-4


FAMILY_CASES = [("benign", 60, 2000, 64, 3), ("benign", 40, 500, 48, 4), ("benign", 40, 500, 200, 1), ("benign", 40, 500, 4, 0),
                ("saturated", 60, 2000, 64, 3), ("saturated", 40, 500, 32, 2), ("zero", 60, 2000, 64, 3), ("zero", 40, 500, 128, 1),
                ("benign", 40, 37, 64, 3), ("benign", 40, 300, 32, 3)]


@pytest.mark.parametrize("family,U,I,d,S", FAMILY_CASES)
def test_float32_model_passes_the_rule_on_every_input_family(family, U, I, d, S):
    """Plain float32 torch is inside the tolerance the kernels are held to, the yardstick E32 stays below its cap (so the rule
    cannot go slack), every score is finite and in [0, 1], and an all-zero head block gives cosine 0."""
    Y = sm.make_table(family, U, I, d, S, seed=d + S)
    users = torch.randperm(U, generator=torch.Generator().manual_seed(1))[:33]
    for ptype, fusion in sm.PAIRS:
        if S == 0 and fusion != "rubi":
            continue
        for mask in sorted({(1 << S) - 1, 0b101 & ((1 << S) - 1)}):
            ref64 = sm.score_model(Y.double(), U, users, d, S, mask, fusion, ptype)
            ref32 = sm.score_model(Y, U, users, d, S, mask, fusion, ptype)
            assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
            tol, e32 = sm.tolerance(ref64, ref32, fast=False)
            assert sm.worst_error(ref32, ref64) <= tol
            assert tol <= 4 * sm.E32_CAP
            assert bool(torch.isfinite(ref32).all()) and float(ref64.min()) >= 0.0 and float(ref64.max()) <= 1.0
    if family == "zero":
        ub, ib = sm.blocks(Y.double(), U, torch.arange(U), d, S)
        z = sm.cosines(ub, ib)
        assert bool((z[0][1] == 0).all()) and bool((z[0][:, 0] == 0).all()) and bool(torch.isfinite(torch.stack(z)).all())
        assert float(z[S - 1][:, 3].abs().max()) > 1e-3         # the 1e-10 block is above the floor: an ordinary cosine


# --------------------------------------------------------------------------- value mutants
def _mutant(name, Y, U, users, d, S, mask, fusion, ptype):
    ub, ib = sm.blocks(Y, U, users, d, S)
    I = ib.shape[0]
    if name == "tail_tile_from_item_i_minus_1":          # the last 16-item tile reads row i - 1
        idx = torch.arange(I)
        t0 = (I - 1) // 16 * 16
        idx[t0:] = (idx[t0:] - 1).clamp_min(0)
        ib = ib[idx]
    a = sm.logits(ub, ib)
    un = [sm.unit(ub[:, h]) for h in range(1, 1 + S)]
    it = [sm.unit(ib[:, h]) for h in range(1, 1 + S)]
    if name == "norm_of_next_user":
        nxt, _ = sm.blocks(Y, U, (users + 1) % U, d, S)
        un[0] = ub[:, 1] / nxt[:, 1].norm(dim=-1, keepdim=True).clamp_min(sm.EPS)
    if name == "no_norm_floor":
        un = [ub[:, h] / ub[:, h].norm(dim=-1, keepdim=True) for h in range(1, 1 + S)]
        it = [ib[:, h] / ib[:, h].norm(dim=-1, keepdim=True) for h in range(1, 1 + S)]
    if name == "item_heads_1_2_swapped":
        it[1], it[2] = it[2], it[1]
    z = [u @ i.T for u, i in zip(un, it)]
    if name == "last_k_term_dropped":
        z[S - 1] = un[S - 1][:, :-1] @ it[S - 1][:, :-1].T

    def fuse(x):
        if name == "rubi_ignores_mask" and fusion == "rubi":
            return sm.fuse(x, z, (1 << S) - 1, fusion)
        if name == "hm_honours_mask" and fusion == "hm":
            return sm.fuse(x, [zh for h, zh in enumerate(z) if (mask >> h) & 1], mask, fusion)
        return sm.fuse(x, z, mask, fusion)

    ui = torch.sigmoid(a)
    if ptype == "normal":
        return ui if name == "normal_with_one_sigmoid" else torch.sigmoid(ui)
    if ptype == "TE":
        return torch.sigmoid(fuse(ui))
    m = ui.mean(-1, keepdim=True)
    if name == "mean_over_I_minus_1":
        m = ui.sum(-1, keepdim=True) / (I - 1)
    if name == "nde_from_ui":
        m = ui
    return torch.sigmoid(fuse(ui) - fuse(m))


# mutant -> the cases meant to catch it: (family, U, I, d, S, head_mask, fusion, predict type)
MUTANTS = {
    "last_k_term_dropped": [("benign", 40, 300, 64, 3, 0b111, "rubi", "TE"), ("benign", 40, 300, 200, 1, 0b1, "sum", "TIE")],
    "item_heads_1_2_swapped": [("benign", 40, 300, 64, 3, 0b111, "hm", "TE"), ("benign", 40, 300, 32, 3, 0b101, "rubi", "TIE")],
    "norm_of_next_user": [("benign", 40, 300, 64, 3, 0b111, "sum", "TIE"), ("benign", 40, 300, 48, 1, 0b1, "rubi", "TE")],
    "rubi_ignores_mask": [("benign", 40, 300, 64, 3, 0b101, "rubi", "TE"), ("benign", 40, 300, 64, 1, 0b0, "rubi", "TIE")],
    "hm_honours_mask": [("benign", 40, 300, 64, 3, 0b101, "hm", "TE"), ("benign", 40, 300, 64, 1, 0b0, "hm", "TIE")],
    "nde_from_ui": [("benign", 40, 300, 64, 3, 0b111, "rubi", "TIE"), ("benign", 40, 300, 64, 3, 0b111, "hm", "TIE")],
    "mean_over_I_minus_1": [("benign", 40, 37, 64, 3, 0b111, "rubi", "TIE"), ("benign", 40, 300, 64, 3, 0b111, "sum", "TIE"),
                            ("benign", 40, 300, 64, 3, 0b111, "hm", "TIE")],
    "normal_with_one_sigmoid": [("benign", 40, 300, 64, 3, 0b111, "rubi", "normal")],
    "no_norm_floor": [("zero", 40, 300, 64, 3, 0b111, "rubi", "TE"), ("zero", 40, 300, 64, 3, 0b111, "sum", "TIE")],
    "tail_tile_from_item_i_minus_1": [("benign", 40, 37, 64, 3, 0b111, "rubi", "TE"), ("benign", 40, 300, 48, 0, 0b0, "rubi", "normal")],
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_rule_rejects_value_mutants(name):
    """Each mutant, evaluated in float64, misses the EXACT and the FAST tolerance on its cases -- and the unmutated path of the
    same function passes them (so it is the mutation that is caught, not the re-composition)."""
    for family, U, I, d, S, mask, fusion, ptype in MUTANTS[name]:
        Y = sm.make_table(family, U, I, d, S, seed=7)
        users = torch.randperm(U, generator=torch.Generator().manual_seed(2))[:33]
        ref64 = sm.score_model(Y.double(), U, users, d, S, mask, fusion, ptype)
        ref32 = sm.score_model(Y, U, users, d, S, mask, fusion, ptype)
        tol, _ = sm.tolerance(ref64, ref32, fast=True)
        assert sm.worst_error(_mutant("none", Y.double(), U, users, d, S, mask, fusion, ptype), ref64) <= 1e-15
        err = sm.worst_error(_mutant(name, Y.double(), U, users, d, S, mask, fusion, ptype), ref64)
        assert err > tol, (name, family, I, d, S, fusion, ptype, err, tol)

