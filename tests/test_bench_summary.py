"""bench.py's compact line on a synthetic record (CPU): the tile summary's
worst-run and harness-stall fields, and that a malformed record costs only
its own summary, never the line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _run(p50, p99, late=0.0, gap=0.0):
    return {"p50_us": p50, "p99_us": p99, "p99_over_p50": p99 / p50, "frags_per_s": 1.0, "offered_frags_per_s": 1.0,
            "txns_per_s": 1.0, "stalls_us": {"producer_late_max": late, "tile_pass_max": 10.0, "consumer_gap_max": gap}}


def _load(runs):
    worst, clean, nst = bench.worst_of(runs)
    med = sorted(runs, key=lambda x: x["p50_us"])[1]
    return {"p50_us": med["p50_us"], "worst_p99_us": worst["p99_us"], "worst_p99_over_p50": worst["p99_over_p50"],
            "harness_stalled_runs": nst, "worst_p99_over_p50_unstalled": clean, "runs": runs}


def _tile():
    ok = [_run(1000, 1100), _run(1010, 1120), _run(990, 1090)]
    stalled = [_run(1000, 1100), _run(1000, 9000, late=5000.0), _run(1005, 1150)]
    rr_ok = {"saturated_frags_per_s": 5e7, "saturated_steady_frags_per_s": 5.2e7, "check_mismatches": 0,
             "roofline": {"frac": 0.3, "frac_steady": 0.31}, "at_50%": _load(ok), "at_80%": _load(stalled)}
    rr_ok["p99_within_2_5x_p50"] = False
    rr_ok["p99_within_2_5x_p50_unstalled"] = True
    tx = {"batch_max": 4096, "saturated_txns_per_s": 8e6, "saturated_verifies_per_s": 5e7,
          "saturated_steady_verifies_per_s": 5.1e7, "check_mismatches": 0, "at_50%": _load(ok), "at_80%": _load(ok),
          "p99_within_2_5x_p50": True, "p99_within_2_5x_p50_unstalled": True}
    return {"rows": [{"batch_max": 4096, "zero_copy": rr_ok}], "all_checks_pass": True,
            "every_row_p99_within_2_5x_p50": False, "every_row_p99_within_2_5x_p50_unstalled": True,
            "every_row_p50_nondecreasing_with_load": True, "frags_per_run": 1 << 25,
            "txn_framing": {"rows": [tx]}}


def _out(tile):
    return {"metric": "m", "value": 1.0, "unit": "verifies/s", "n_gpus": 1, "steps": 1, "warmup": 1, "ms_per_step": 1.0,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int64", "data": "synthetic",
            "config": {"workload": "w"}, "stream_tile": tile}


def test_worst_of_separates_harness_stalls():
    runs = [_run(1000, 1100), _run(1000, 9000, late=5000.0), _run(1000, 1200, gap=3000.0)]
    worst, clean, nst = bench.worst_of(runs)
    assert worst["p99_us"] == 9000 and nst == 2 and abs(clean - 1.1) < 1e-9
    worst, clean, nst = bench.worst_of([_run(1000, 9000, late=5000.0)] * 3)
    assert clean is None and nst == 3


def test_compact_line_tile_summary_fields():
    line = json.loads(bench.compact_line(_out(_tile()), "d.json"))
    st = line["stream_tile"]
    assert st["every_row_worst_p99_within_2_5x_p50"] is False
    assert st["every_row_worst_p99_within_2_5x_p50_runs_without_harness_stalls"] is True
    row = st["rows"][0]
    assert row["worst_x_80"] == 9.0 and row["stalled_runs_80"] == 1 and row["worst_x_unstalled_80"] == 1.14
    assert "stalled_runs_50" not in row
    assert st["txn_framing"][0]["worst_x_50"] == 1.11


def test_malformed_tile_record_costs_only_its_summary():
    tile = _tile()
    del tile["rows"][0]["zero_copy"]["at_80%"]
    line = json.loads(bench.compact_line(_out(tile), "d.json"))
    assert line["value"] == 1.0 and "summary_error" in line["stream_tile"]


def test_unstalled_check_fails_when_every_run_stalled():
    """A load with no stall-free run cannot pass the harness-stall view of the tail check."""
    import bench
    ok = {"worst_p99_over_p50_unstalled": 1.2}
    assert bench.unstalled_ok([ok, ok])
    assert not bench.unstalled_ok([ok, {"worst_p99_over_p50_unstalled": None}])
    assert not bench.unstalled_ok([ok, {"worst_p99_over_p50_unstalled": 2.6}])


def test_roofline_from_rocprof_and_held_clock(tmp_path, monkeypatch):
    """The line's profiler-timed DSM fraction and held clock: the committed rocprofv3 averages of the stage's
    launches, GRBM_GUI_ACTIVE / 8 XCDs over k_dsmp's duration; the traffic raw and 2x-corrected."""
    import json
    import numpy as np
    import bench
    csv = tmp_path / "r99_rocprof_kernel_stats.csv"
    csv.write_text('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
                   '"k_dsmp(unsigned int)",2,26000000,13000000.0,90,1,1,0\n'
                   '"k_ai(unsigned int)",2,1000000,500000.0,5,1,1,0\n'
                   '"k_fin(unsigned int)",2,200000,100000.0,1,1,1,0\n')
    pmc = tmp_path / "r99_pmc_latest.json"
    pmc.write_text(json.dumps({"_sigs_per_launch": 1 << 20, "k_dsmp": {
        "counters": {"GRBM_GUI_ACTIVE": 8 * 2.2e9 * 13e-3},
        "derived": {"hbm_bytes_per_launch": 2.0e10, "fetch_kb_raw": 9.0e6, "write_kb_raw": 1.0e6}},
        **{k: {"counters": {}, "derived": {"hbm_bytes_per_launch": 0.0, "fetch_kb_raw": 0.0, "write_kb_raw": 0.0}}
           for k in ("k_ai", "k_fin")}}))
    monkeypatch.setattr(bench, "rocprof_stats_path", lambda: str(csv))
    monkeypatch.setattr(bench, "pmc_summary_path", lambda: str(pmc))
    assert abs(bench.rocprof_stage_ms(["k_ai", "k_dsmp", "k_fin"])[0] - 13.6) < 1e-9
    assert abs(bench.held_clock_ghz("k_dsmp") - 2.2) < 1e-9
    n = 1 << 20
    st = np.zeros((3, n), np.uint32)
    st[0] = 250
    st[1] = 42
    st[2] = 43
    r = bench.dsm_roofline(st, 13.0, n, kernel="k_ai+k_dsmp+k_fin")
    assert abs(r["frac_rocprof"] / r["frac"] - 13.0 / 13.6) < 1e-9
    assert abs(r["frac_at_held_clock"] / r["frac"] - 2.4 / 2.2) < 1e-9
    assert r["traffic"] == 2.0e10 and r["traffic_raw"] == 1.0e7 * 1024


def test_stalled_runs_are_topped_up_and_left_out_of_the_median():
    """A producer stall on two of three paced runs: more runs until three are
    stall-free (at most TOPUP_MAX), the p50 is their median, and every run --
    stalled and extra ones too -- stays in the all-runs tail check."""
    rs = [_run(700, 800), _run(150000, 320000, late=300000.0), _run(152000, 330000, late=310000.0)]
    fresh = iter([_run(710, 790), _run(690, 770), _run(720, 800)])
    extra = bench.top_up(rs, lambda: next(fresh))
    assert extra == 2 and len(rs) == 5
    assert bench.p50_run(rs)["p50_us"] == 700                      # median of 700, 710, 690
    worst, clean, nst = bench.worst_of(rs)
    assert nst == 2 and worst["p99_us"] == 330000 and clean < 1.2  # the stalled runs still set the all-runs tail
    # at most TOPUP_MAX extra runs, then the median over whatever is clean
    rs2 = [_run(1000, 1100, late=5000.0)] * 3
    stalled = iter([_run(1000, 1100, late=5000.0)] * bench.TOPUP_MAX)
    assert bench.top_up(rs2, lambda: next(stalled)) == bench.TOPUP_MAX
    assert bench.p50_run(rs2)["p50_us"] == 1000                    # none clean: the median of all
    # three clean runs: nothing extra
    rs3 = [_run(600, 700), _run(610, 700), _run(620, 700)]
    assert bench.top_up(rs3, lambda: None) == 0 and bench.p50_run(rs3)["p50_us"] == 610


def test_bench_batch_flips_one_message_bit_in_a_seeded_sixteenth(monkeypatch):
    """The bench batch: n // 16 signatures, the same ones on every call, differ from the signed batch in exactly
    one bit of their own message; keys, signatures and layout are untouched; the default leaves the batch whole."""
    import numpy as np
    import bench
    from firedancer_amd import workload
    n, m = 1 << 12, 200

    def signed(n, m, seed):
        rng = np.random.default_rng(seed)
        return (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 64), dtype=np.uint8),
                (np.arange(n) * m).astype(np.uint32), np.full(n, m, np.uint32),
                rng.integers(0, 256, n * m + 1, dtype=np.uint8))
    monkeypatch.setattr(workload, "sig_batch", signed)
    whole = bench.make_workload(n, m, 1000)
    a, b = bench.make_workload(n, m, 1000, bench.FLIP_ONE_IN), bench.make_workload(n, m, 1000, bench.FLIP_ONE_IN)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(whole, signed(n, m, 1000)))
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], whole[:4]))
    d = np.nonzero(a[4] != whole[4])[0]
    assert d.size == n // bench.FLIP_ONE_IN == np.unique(d // m).size and d.max() < n * m
    assert all(bin(int(x)).count("1") == 1 for x in a[4][d] ^ whole[4][d])
    other = bench.make_workload(n, m, 1001, bench.FLIP_ONE_IN)[4]
    assert not np.array_equal(np.nonzero(other != signed(n, m, 1001)[4])[0] // m, d // m)


def test_dump_outputs_float32_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 files named after the arrays (other ranks' with their rank), whole when they fit
    their share of the cap, else the same sorted sample on every call."""
    import numpy as np
    import bench
    err = (np.arange(1000) % 7 - 3).astype(np.int8)
    bench.dump_outputs(str(tmp_path / "a"), {"verdicts": err})
    got = np.load(tmp_path / "a" / "verdicts.npy")
    assert got.dtype == np.float32 and np.array_equal(got, err.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 2 * 2 * 100)   # 2 ranks x 2 arrays x 100 elements
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"txn_verdicts": err[:100], "sig_verdicts": err}, rank=1, world=2)
    whole = np.load(tmp_path / "b" / "txn_verdicts_rank1.npy")
    cut = np.load(tmp_path / "b" / "sig_verdicts_rank1.npy")
    assert np.array_equal(whole, err[:100].astype(np.float32))
    assert cut.dtype == np.float32 and cut.shape == (100,)
    assert np.array_equal(cut, np.load(tmp_path / "c" / "sig_verdicts_rank1.npy"))
    total = sum(os.path.getsize(tmp_path / "b" / f) - 128 for f in os.listdir(tmp_path / "b"))
    assert total <= bench.DUMP_MAX_BYTES // 2


def test_plain_run_line_and_options(monkeypatch, capsys):
    """A plain run's line: the headline keys, no side file; --full and --dump-outputs parse, off by default."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(bench, "write_detail", lambda out, args: (_ for _ in ()).throw(AssertionError("side file")))
    out = {k: v for k, v in _out(None).items() if k != "stream_tile"}
    bench.emit(out, args)
    line = json.loads(capsys.readouterr().out.strip())
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["detail"] is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"


def test_full_run_without_the_compiled_reference_says_so(monkeypatch, tmp_path, capsys):
    """--full where oracle/_ref was not built: no CPU baseline, named in the line; never the port in its place."""
    import bench
    monkeypatch.setattr(bench, "REF_BATCH_SO", str(tmp_path / "missing.so"))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    args = bench.parse()
    bench.cpu_baseline_or_skip(args)
    assert args.no_cpu is True
    monkeypatch.setattr(bench, "write_detail", lambda out, args: "d.json")
    bench.emit({k: v for k, v in _out(None).items() if k != "stream_tile"}, args)
    line = json.loads(capsys.readouterr().out.strip())
    assert "cpu_baseline" not in line and "missing.so" in line["cpu_baseline_skipped"]
    # a plain run never needs it
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    args = bench.parse()
    bench.cpu_baseline_or_skip(args)
    assert args.no_cpu is False and not hasattr(args, "cpu_skipped")
