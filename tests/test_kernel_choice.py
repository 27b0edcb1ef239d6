"""The one rule that picks a sim's physics kernel form (isaacgymenv_amd/csrc/gs_kernel_choice.h), over every
combination of its seven inputs.

A stand-alone program that includes only that header prints the whole table; the expectation below was written from
the three functions the rule replaces (gs_sim_set_model's selection, kernel_select and the fallback of
gs_sim_set_self_collision in gs_capi.hip before the split), not from the rule's own output.  CPU only.
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaacgymenv_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "gs_kernel_choice.h"
int main() {
  const int wants[4] = {0, 1, 2, 4};
  for (int host = 0; host < 2; ++host)
    for (int compiled = 0; compiled < 2; ++compiled)
      for (int team = 0; team < 2; ++team)
        for (int limits = 0; limits < 2; ++limits)
          for (int want : wants)
            for (int drive = 0; drive < 2; ++drive)
              for (int table = 0; table < 2; ++table) {
                const KernelChoice c =
                    kernel_choice({host != 0, compiled != 0, team != 0, limits, want, drive, table != 0});
                std::printf("%d %d %d %d %d %d %d|%d|%s\n", host, compiled, team, limits, want, drive, table, c.variant,
                            c.refusal ? c.refusal : "");
              }
  return 0;
}
"""

# the refusal texts as gs_capi.hip had them (%s: the topology signature, or the entry point that asked)
HOST_RUNTIME = ("gs_sim_set_model: the runtime-sized kernel is a GPU kernel and no host solver is compiled for this "
                "topology (add it with tools/gen_topologies.py): %s")
NOT_COMPILED = ("gs_sim_set_model: kernel_variant 1 / 2 requested but topology %s is not compiled (the runtime-sized "
                "kernel is variant 4)")
TEAM_ON_HOST = "gs_sim_set_model: the lane-team kernel is a GPU kernel (host sim)"
NO_TEAM = "gs_sim_set_model: no lane-team kernel for this topology / joint limits"
NO_DRIVES = "%s: the lane-team kernel (kernel_variant 2) has no joint drives"
NO_DRIVES_OR_TABLE = "%s: the lane-team kernel (kernel_variant 2) has no joint drives or per-actor dof properties"

ANY = None
# (host, compiled topology, lane-team entry, joint limits, kernel_variant, drives, per-actor table) -> variant or
# refusal; ANY matches both values (all four of kernel_variant), a tuple the listed ones.  Every combination matches
# one row.
TABLE = [
    # host sims: compiled topologies only, never the lane team; drives and tables change nothing
    ((1, 0, ANY, ANY, ANY, ANY, ANY), HOST_RUNTIME),
    ((1, 1, ANY, ANY, 2, ANY, ANY), TEAM_ON_HOST),
    ((1, 1, ANY, ANY, (0, 1, 4), ANY, ANY), 3),
    # no compiled topology: the runtime-sized kernel, which has limits, drives and per-actor tables
    ((0, 0, ANY, ANY, (1, 2), ANY, ANY), NOT_COMPILED),
    ((0, 0, ANY, ANY, (0, 4), ANY, ANY), 4),
    # kernel_variant 4 on a compiled topology
    ((0, 1, ANY, ANY, 4, ANY, ANY), 4),
    # kernel_variant 1
    ((0, 1, ANY, ANY, 1, ANY, ANY), 1),
    # kernel_variant 2: the lane team or a refusal
    ((0, 1, 0, ANY, 2, ANY, ANY), NO_TEAM),
    ((0, 1, 1, 1, 2, ANY, ANY), NO_TEAM),
    ((0, 1, 1, 0, 2, 0, 0), 2),
    ((0, 1, 1, 0, 2, 1, 0), NO_DRIVES),
    ((0, 1, 1, 0, 2, ANY, 1), NO_DRIVES_OR_TABLE),
    # auto: the lane team where the topology has one and nothing in use is beyond it
    ((0, 1, 0, ANY, 0, ANY, ANY), 1),
    ((0, 1, 1, 1, 0, ANY, ANY), 1),
    ((0, 1, 1, 0, 0, 0, 0), 2),   # ... which is also where a sim returns once its drive gains are zero again
    ((0, 1, 1, 0, 0, 1, 0), 1),   # team topology plus drives
    ((0, 1, 1, 0, 0, ANY, 1), 1),
]


def _expected():
    exp = {}
    for combo in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2, 4), (0, 1), (0, 1)):
        hits = [res for pat, res in TABLE
                if all(p is ANY or (v in p if isinstance(p, tuple) else v == p) for p, v in zip(pat, combo))]
        assert len(hits) == 1, (combo, hits)
        exp[combo] = hits[0]
    return exp


def test_kernel_choice_table(tmp_path):
    from isaacgymenv_amd import build
    try:
        hipcc = build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    src = tmp_path / "choice.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "choice"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        combo, variant, refusal = line.split("|")
        assert (int(variant) == 0) == bool(refusal), line
        got[tuple(int(x) for x in combo.split())] = refusal or int(variant)
    exp = _expected()
    assert len(exp) == 256 and got.keys() == exp.keys()
    wrong = {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]}
    assert not wrong, wrong
