"""The pt_gs_k step's paired exps and logs inside the run kernels, bit for bit against the oracle.

The step evaluates every two independent exps side by side (kmath::exp2, device/pt_dev.h: Priestley-Taylor's
saturation-pressure exp with actual evapotranspiration's, kirchner_f's two exps), each pair with one merged test
for the general path; its logs are single (pairing Priestley-Taylor's log with Kirchner's opening log(q) was
measured and left out; the inputs below cover that pairing too, should it return). The synthetic
region of the other parity tests never leaves the fast domains, so this region is made to:
  - the initial Kirchner q per cell is drawn from {1.0, 1e-5, 9.9e-6, 0.0, 5e-324, 1e-310, 1e300}: both sides of
    Kirchner's clamp q < 1e-5 ahead of its opening log, and a q whose actual_evapotranspiration exp argument
    -3 q / ae_scale is beyond exp's fast domain while its partner in the pair is inside;
  - some temperatures sit just above -245.425 degC, where ck2 T / (ck3 + T) is large negative: the saturation
    pressure's exp takes the general path and returns 0, and log(10 vp / T_k) = log(0) takes the log's;
  - the last step's temperature row is NaN (both domain tests fail on NaN) over the first 200 cells; the other 100
    cells keep a finite final state, so that the final-state comparison is not NaN against NaN throughout.
300 cells x 48 steps, on the 256-lane and the 64-lane instance, each as the general kernel (all 8 series of the
full collector) and as the lean kernel (the discharge collector), selected as tests/test_ptgsk_instances.py selects
them (the launcher's knob is read once per process, hence a child process per case); the final state in every case.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from shyft_amd import synthetic
from tests import engines

pytestmark = pytest.mark.gpu

N, T = 300, 48
N_NAN = 200  # the NaN temperature row covers these cells; the other 100 end the run with a finite state to compare
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q0 = (1.0, 1e-5, 9.9e-6, 0.0, 5e-324, 1e-310, 1e300)
T_COLD = (-245.0, -245.42, -240.0)  # ck2 T / (ck3 + T) = -1.0e4, -8.8e5, -789 (ck2 = 17.84362, ck3 = 245.425)

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from shyft_amd import synthetic
from tests import engines
d = np.load(sys.argv[2])
g = engines.run("hip", d["geo"], d["params"], d["state"], synthetic.T0_2015_US, synthetic.HOUR_US, d["forcing"],
                full=sys.argv[3] == "full")
np.savez(sys.argv[4], series=np.asarray(g["full"] if sys.argv[3] == "full" else g["main"]), st=np.asarray(g["state"]))
'''


def region_inputs():
    geo = synthetic.geo11(N)
    f = synthetic.forcing(N, 0, T, synthetic.SEED).copy()
    rng = np.random.default_rng(114)
    state = synthetic.default_ptgsk_state(N)
    state[:, 8] = np.asarray(Q0)[rng.integers(0, len(Q0), N)]
    state[:len(Q0), 8] = Q0  # every value at least once
    # cold cells: every 7th cell at steps 0, 1, 20 and 40 (so that a cold step meets every initial q and later states)
    for k, t in enumerate((0, 1, 20, 40)):
        f[0, t, (k % 3)::7] = T_COLD[k % 3]
    f[0, T - 1, :N_NAN] = np.nan
    return geo, synthetic.default_ptgsk_parameters(), state, f


def path_counts(state, f):
    """How many cell-steps take each side of the tests the pairs merge, from the inputs alone (numpy)."""
    q0 = state[:, 8]
    temp, rh = f[0], f[3]
    neg = temp < 0
    arg = np.where(neg, 17.84362, 17.08085) * temp / (np.where(neg, 245.425, 234.175) + temp)
    with np.errstate(all="ignore"):
        vp = 0.610780 * np.exp(arg) * rh
        larg = 10 * vp / (temp + 273.15)
    return {"clamped": int((q0 < 0.00001).sum()), "not clamped": int((q0 >= 0.00001).sum()),
            "ae exp beyond": int((np.abs(-q0 * 3.0 / 1.5) > 708.0).sum()),
            "pt exp beyond": int((~(np.abs(arg) <= 708.0)).sum()), "pt exp inside": int((np.abs(arg) <= 708.0).sum()),
            "pt log beyond": int((~((larg >= 2.2250738585072014e-308) & (larg <= 1.7976931348623157e308))).sum()),
            "pt log inside": int(((larg >= 2.2250738585072014e-308) & (larg <= 1.7976931348623157e308)).sum())}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    geo, params, state, f = region_inputs()
    counts = path_counts(state, f)
    assert all(v > 0 for v in counts.values()), counts
    c = engines.run("oracle", geo, params, state, synthetic.T0_2015_US, synthetic.HOUR_US, f, full=True)
    full, st = np.asarray(c["full"]), np.asarray(c["state"])
    assert np.isnan(full[:, T - 1, :N_NAN]).any() and np.isfinite(full[:, :T - 1]).all() and np.isfinite(st[N_NAN:]).all()
    inp = tmp_path_factory.mktemp("pairs_run") / "in.npz"
    np.savez(inp, geo=geo, params=params, state=state, forcing=f)
    return str(inp), full, st


@pytest.mark.parametrize("collector", ["full", "discharge"])
@pytest.mark.parametrize("env", [{"SHYFT_PTGSK_WAVES": "4"}, {}], ids=["w4", "default"])
def test_pairs_run_bitexact(env, collector, case, tmp_path):
    inp, full, st = case
    out = tmp_path / "g.npz"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, inp, collector, str(out)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    g = np.load(out)
    ref = full if collector == "full" else full[:2]
    for name, a, b in (("response series", g["series"], ref), ("final state", g["st"], st)):
        assert a.shape == b.shape, f"{name}: shape {a.shape} against {b.shape}"
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        assert same.all(), f"{json.dumps(env)} {collector} {name}: {int((~same).sum())} values differ"
