"""The job sets of tests/snow_cases.py on the CPU: the Python restatements of one hbv_snow and one hbv_physical_snow
step reproduce the oracle's single-step entries bit for bit and raise on exactly the jobs where the oracle raises; the
clean jobs of every stack reach every label at every time step; and the shares of raising and of trivially resetting
jobs stay under their caps. The GPU file runs these same jobs as the cells of a region."""
import numpy as np
import pytest

from tests import snow_cases as sc

KINDS = {"hs": sc.HS_LABELS, "hps": sc.HPS_LABELS}
MIN_JOBS = 8


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("dt_name", list(sc.DTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_restatement_equals_the_oracle_step_bit_for_bit(kind, dt_name):
    jobs = sc.snow_jobs(kind, dt_name)
    dt_us = sc.DTS[dt_name]
    for i in range(len(jobs["k"])):
        k, row, f = int(jobs["k"][i]), jobs["row"][i], tuple(jobs["f"][i])
        what = f"{kind} {dt_name} job {i} ({jobs['tag'][i]}, set {sc.set_names()[k]}): row {row.tolist()} forcing {f}"
        new, out, labels = sc._run_python(kind, k, row, dt_us, f)
        try:
            want, want_out = sc._run_oracle(kind, k, row, dt_us, f)
        except RuntimeError as e:
            assert "Negative outflow" in str(e), what
            assert sc.RAISE in labels, "the oracle raises, the restatement does not: " + what
            continue
        assert sc.RAISE not in labels, "the restatement raises, the oracle does not: " + what
        assert _bits_equal(new, want), f"state differs: {what}\n{new.tolist()}\n{want.tolist()}"
        assert _bits_equal(out, want_out), f"response differs: {what}: {out!r} vs {want_out!r}"
        assert labels <= set(KINDS[kind]), labels - set(KINDS[kind])


@pytest.mark.parametrize("dt_name", list(sc.DTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_clean_jobs_reach_every_label_and_stay_under_the_caps(kind, dt_name, capsys):
    """Every label of the routine is reached by at least 8 jobs that do not raise (none is unreachable without
    raising); at most 15 % of the jobs raise, at most 25 % end in the trivial reset, and the mass-balance clamp
    (swe = total_water) has 8 jobs of its own."""
    jobs = sc.snow_jobs(kind, dt_name)
    n = len(jobs["k"])
    counts = sc.label_counts(jobs, KINDS[kind])
    n_raise = int(jobs["raises"].sum())
    n_reset = sum("reset" in L for L in jobs["labels"])
    with capsys.disabled():
        print(f"\n{kind} {dt_name}: {n} jobs, {n_raise} raise, {n_reset} reset; clean jobs per label: {counts}")
    assert n < 3000 and n % 64 != 0
    low = {lab: c for lab, c in counts.items() if c < MIN_JOBS}
    assert not low, low
    assert n_raise <= 0.15 * n and n_reset <= 0.25 * n
    assert n_raise >= 8                      # the raising side is there to be mixed in
    assert counts["clamp"] >= MIN_JOBS
    # bin counts: states that come undistributed, with the set's count and with another set's
    nbc = 2 if kind == "hs" else 3
    sets = sc.hs_sets() if kind == "hs" else sc.hps_sets()
    own = np.array([len(sets[k]["I"]) for k in jobs["k"]])
    nbs = jobs["row"][:, nbc].astype(int)
    assert (nbs == 0).sum() >= MIN_JOBS and (nbs == own).sum() >= MIN_JOBS
    assert ((nbs != 0) & (nbs != own)).sum() >= MIN_JOBS
    for k in range(len(sets)):               # every set has clean jobs of its own (the uniform launch instances)
        assert ((jobs["k"] == k) & ~jobs["raises"]).sum() >= 40, sc.set_names()[k]


@pytest.mark.parametrize("dt_name", list(sc.DTS))
def test_hbv_stack_jobs_reach_every_branch_of_the_rest_of_the_step(dt_name, capsys):
    """sm on either side of lp, the beta == 2 shortcut and pow, the soil outflow clamp, sm clamped at 0, q12 at 0 and
    above, the upper tank on either side of uz1: labels from the oracle's response to the hbv_stack jobs."""
    case = sc.region_case("hbv_stack", dt_name)
    ref = sc.run_oracle_region("hbv_stack", case)
    labels = sc.hbv_tail_labels(case, ref)
    counts = {lab: sum(lab in L for L in labels) for lab in sc.HBV_TAIL_LABELS}
    with capsys.disabled():
        print(f"\nhbv_stack {dt_name}: {len(labels)} clean jobs; per label: {counts}")
    low = {lab: c for lab, c in counts.items() if c < MIN_JOBS}
    assert not low, low


@pytest.mark.parametrize("dt_name", list(sc.DTS))
@pytest.mark.parametrize("stack", sc.STACKS)
def test_oracle_region_of_clean_jobs_runs_and_of_raising_jobs_raises(stack, dt_name):
    """the oracle's region run (the GPU file's reference) leaves every clean job's snow state as the single-step
    restatement does, so the stack's parameter rows carry the sets; and it raises on the raising jobs"""
    jobs = sc.stack_jobs(stack, dt_name)
    clean = sc.region_case(stack, dt_name)
    assert clean["geo"].shape[0] % 64 != 0 and clean["geo"].shape[0] < 3000
    ref = sc.run_oracle_region(stack, clean)
    kind = "hps" if stack == "pt_hps_k" else "hs"
    for c, i in enumerate(clean["jobs"]):
        new = sc._run_python(kind, int(jobs["k"][i]), jobs["row"][i], sc.DTS[dt_name], jobs["f"][i])[0]
        got = ref["state"][c]
        got = np.concatenate([got[0:2], got[5:]]) if stack == "hbv_stack" else got[:len(new)]
        assert _bits_equal(got, new), (stack, dt_name, int(i), jobs["tag"][i])
    for i in np.flatnonzero(jobs["raises"])[:10]:
        with pytest.raises(RuntimeError, match="Negative outflow"):
            sc.run_oracle_region(stack, sc.region_case(stack, dt_name, select=[i]))


@pytest.mark.parametrize("dt_name", list(sc.DTS))
@pytest.mark.parametrize("stack", sc.STACKS)
def test_scripted_sequences_pass_through_every_event_and_run_clean(stack, dt_name):
    """8 to 12 steps in which one branch's output is the next step's input: together the sequences pass through
    snowfall onto partial cover, partial melt, rain on partial cover, refreeze, melt to nothing, the reset and snowfall
    again (hbv_physical_snow: also the sp[idx-1] = sp[idx] assignment with an integration over it in the next step),
    and the oracle's region runs them without raising."""
    case = sc.sequence_case(stack, dt_name)
    assert 8 <= case["forcing"].shape[1] <= 12
    seen = set().union(*case["events"])
    required = sc.HPS_SEQ_REQUIRED if stack == "pt_hps_k" else sc.SEQ_REQUIRED
    assert set(required) <= seen, set(required) - seen
    sc.run_oracle_region(stack, case)
