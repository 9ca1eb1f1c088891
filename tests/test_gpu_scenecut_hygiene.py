"""Kernel hygiene of the scene-statistics entry point (scenecut.hip), with the
helpers and the five steps of tests/hygiene.py (tests/test_gpu_kernel_hygiene.py
explains them), as tests/test_gpu_chroma_hygiene.py uses them.

dcvc_scene_stats takes raw pointers and scalars, so the walk of
test_gpu_kernel_hygiene.py, which looks for tensor-struct parameters, does not
see it; the table below covers it and a CPU test walks scenecut.hip for an
entry point it misses.

Per entry (depths 8 and 10; planes that start on a 16-byte boundary, planes
that need a head and a tail, planes that are not equally aligned): both planes
sit in buffers with 64 guard elements on both sides that hold zero, the type's
minimum and its maximum; the workspace is guarded and pre-filled the same way;
out2 has a canary around it and inside.  The two words equal the restatement
(tests/scenecut_ref.py), are identical across the fills, across two runs and
after dcvc_debug_poison_lds / dcvc_debug_poison_vgpr, and no byte outside a
view is written.
"""
import os
import re

import numpy as np
import pytest
import torch

from dcvc_amd import hip as K
from tests import hygiene as HY
from tests import scenecut_ref as R
from tests.hygiene import seeded

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 37 * 53 + 5               # more than one block; no multiple of a 16-byte piece at either depth
DEPTHS = (8, 10)
# (samples cur starts after its guard, samples prev does): aligned, equal heads, unequal
OFFSETS = {"aligned": (0, 0), "head and tail": (3, 3), "unequal": (1, 2)}
TABLE = {}


SIZED_BY = "dcvc_scene_stats_workspace"     # launches nothing: every case sizes its guarded scratch by it


def entry(name, symbol, fn):
    assert name not in TABLE
    TABLE[name] = (fn, (symbol,))


def smp(E, key, d, n):
    """Samples in [0, max_val] as the device tensors hold them: uint8, or the
    bits of uint16 as int16."""
    def make():
        a = torch.randint(0, 1 << d, (n,), generator=seeded(f"{key}{d}")).numpy()
        return torch.from_numpy(a.astype(np.uint8) if d == 8 else a.astype(np.uint16).view(np.int16))
    return E.const(f"{key}{d}{n}", make)


def stats_case(E, d, off):
    oa, ob = off
    a, b = smp(E, "cur", d, N + oa).clone(), smp(E, "prev", d, N + ob).clone()
    # the samples before a plane's start belong to its surroundings: they hold the fill like the guards
    HY.fill_(a[:oa], E.fill)
    HY.fill_(b[:ob], E.fill)
    cur, prev = E.raw(a)[oa:], E.raw(b)[ob:]
    ws = E.scratch(int(K.lib().dcvc_scene_stats_workspace()) // 8, torch.int64)
    out = E.yraw("out2", 2, torch.int64)
    E.launch(K.scene_stats, cur, prev, d, ws, out)
    E.ref("out2", lambda: torch.tensor(R.stats(a[oa:].numpy(), b[ob:].numpy(), d), dtype=torch.int64), None)


for _d in DEPTHS:
    for _name, _off in OFFSETS.items():
        entry(f"scene_stats {_name}, {_d} bit", "dcvc_scene_stats", lambda E, d=_d, o=_off: stats_case(E, d, o))


# ---------------------------------------------------------------- the tests
def entry_points():
    """What this table answers for: the extern "C" functions of scenecut.hip."""
    text = open(os.path.join(ROOT, "dcvc_amd", "csrc", "hip", "scenecut.hip")).read()
    names = set(re.findall(r'extern "C" \w+ (dcvc_\w+)\(', text))
    assert "dcvc_scene_stats" in names and SIZED_BY in names, names
    return names


def test_every_scenecut_launcher_has_a_hygiene_case():
    covered = {}
    for name, (_, syms) in TABLE.items():
        for s in syms:
            covered.setdefault(s, []).append(name)
    known = {n: args for n, _, args in K.HIP_SYMBOLS}
    names = entry_points()
    assert names <= set(known), sorted(names - set(known))
    launchers = names - {SIZED_BY}
    assert launchers and all(known[n] for n in launchers) and known[SIZED_BY] == []
    missing = sorted(launchers - set(covered))
    assert not missing, f"scenecut launchers without a hygiene case: {missing}"
    # every extern "C" of the file is a launcher with a case or the size query the cases call
    assert names == set(covered) | {SIZED_BY}
    assert set(covered) <= set(known)
    for s in launchers:
        for d in DEPTHS:
            for o in OFFSETS:
                assert any(f"{o}, {d} bit" in n for n in covered[s]), (s, d, o)
    # none of them is visible to the tensor-struct walk of test_gpu_kernel_hygiene.py
    for n in names:
        assert K.CTensor not in known[n], n
    assert HY.GUARD == 64


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_entry_builds_on_the_cpu(name):
    """Every entry builds its call and its reference without a device (the
    launch skipped): the reference has the shape of the output it is for."""
    fn, _ = TABLE[name]
    env = HY.Env("zero", {}, device=torch.device("cpu"), dry=True)
    fn(env)
    assert env.refs and set(env.refs) <= set(env.outs)
    for out, (ref, _, _) in env.refs.items():
        r = ref()
        assert tuple(r.shape) == tuple(env.values(out).shape), (out, tuple(r.shape))


@gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_kernel_hygiene(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fn, syms = TABLE[name]
    try:
        routes = HY.run_entry(fn, name)
    finally:
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:     # a GPU error poisons the process: launch nothing more
            pytest.exit(f"GPU error, stopping: {e}", returncode=3)
    assert set(routes) == set(syms), (routes, syms)
