"""HoundFakeGym -- TEST INFRASTRUCTURE: tests/fakegym.FakeGym for HoundTerrain.

The stock fake never touches a shoulder, and its thigh contacts (5 % per thigh per simulate) would end most
episodes before a shoulder or the episode limit could.  This subclass thins the thigh contacts and adds rare shoulder
contacts, both from a seeded stream of its own (neither the stock fake's stream nor torch's RNG moves), so that
tests/golden/hound_terrain.npz holds resets by a shoulder alone, a thigh alone, the trunk, and time-outs.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.fakegym import FakeGym


class HoundFakeGym(FakeGym):
    def __init__(self, seed: int = 2024, thigh_keep: float = 0.2, shoulder_p: float = 0.01, **kw):
        super().__init__(seed=seed, **kw)
        self.thigh_keep = thigh_keep  # fraction of the stock fake's thigh contacts that stay
        self.shoulder_p = shoulder_p  # chance per shoulder per simulate of a contact

    def prepare_sim(self, sim):
        ok = super().prepare_sim(sim)
        self.shoulders = [i for i, n in enumerate(sim.asset.art.link_names()) if "shoulder" in n]
        return ok

    def simulate(self, sim):
        super().simulate(sim)
        rng = np.random.RandomState(self.seed + 500000 + sim.t)
        N, nb = sim.N, sim.nb
        cf = sim.cf.view(N, nb, 3)
        for k in self.knees:
            cf[:, k, :] *= torch.from_numpy((rng.rand(N, 1) < self.thigh_keep).astype(np.float32))
        for k in self.shoulders:
            hit = (rng.rand(N, 1) < self.shoulder_p).astype(np.float32)
            cf[:, k, :] = torch.from_numpy(hit * np.array([[1.0, -2.0, 2.0]], dtype=np.float32))


def load_fixture():
    """tests/golden/hound_terrain.npz and hound_terrain_tail.npz (one recording kept as two files) as one dict."""
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = {}
    for name in ("hound_terrain.npz", "hound_terrain_tail.npz"):
        with np.load(os.path.join(golden, name)) as z:
            d.update({k: z[k] for k in z.files})
    return d


def fixture_conditions(d):
    """What tests/golden/hound_terrain.npz must hold (asserted by its generator and re-asserted by the tests that
    use it): the number of env-steps reset by a shoulder contact alone, by a thigh contact alone, by the trunk, by the
    episode limit alone (VecTask's time_outs output stays false: it is taken after the reset zeroed progress), the
    number of push steps and of env-steps without a reset, and the largest |base_height| episode sum.  Contacts are
    read as check_termination reads them: |f| > 1 on the link's row."""
    hit = np.linalg.norm(d["in_contact"].astype(np.float64), axis=-1) > 1.0  # [T, N, links]
    trunk = hit[:, :, int(d["base_index"])]
    thigh = hit[:, :, d["knee_indices"]].any(-1)
    shoulder = hit[:, :, d["base_indices"]].any(-1)
    limit = d["in_progress"] + 1 >= int(d["max_episode_length"]) - 1
    reset = d["reset"] != 0
    assert np.array_equal(reset, trunk | thigh | shoulder | limit), "reset mask is not check_termination's"
    terms = [str(t) for t in d["terms"]]
    return {"shoulder_only": int((shoulder & ~thigh & ~trunk & ~limit).sum()),
            "thigh_only": int((thigh & ~shoulder & ~trunk & ~limit).sum()),
            "trunk": int(trunk.sum()), "time_out": int((limit & ~trunk & ~thigh & ~shoulder).sum()),
            "push": int(d["in_push"].sum()), "no_reset": int((~reset).sum()),
            "base_height_sum": float(np.abs(d["episode_sums"][:, terms.index("base_height")]).max())}


def assert_fixture_conditions(d):
    c = fixture_conditions(d)
    for k, v in c.items():
        assert v > 0, f"hound_terrain.npz holds no {k} case: {c}"
    return c
