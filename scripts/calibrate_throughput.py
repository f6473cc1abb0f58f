"""Calibrations per second of p7x_calibrate_batch for 64 single-sequence models of M = 300, against the path that existed before
it: 64 single-model SequenceDatabase.filters calls plus the Python fits (bench_workloads.Calibrator).  Run from the
repository root on the GPU: python scripts/calibrate_throughput.py  (figures: profiles/r11_calibrate_throughput.md)."""
import sys, time
sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
import numpy as np
import bench_workloads
from pyhmmer_amd import easel, plan7

abc = easel.Alphabet.amino(); bg = plan7.Background(abc)
f = bg.residue_frequencies.astype(np.float64); rng = np.random.default_rng(3)
b = plan7.Builder(abc)
hmms = [b._model(easel.DigitalSequence(abc, name=f"q{i}", sequence=rng.choice(20, size=300, p=f / f.sum()).astype(np.uint8)), bg) for i in range(64)]
plan7._calibrate([plan7.OptimizedProfile(hmms[0], bg, 100)])          # context, resident stream
cal = bench_workloads.Calibrator(abc, device=0)
cal.calibrate(hmms[0].copy())
for rep in range(3):
    t0 = time.perf_counter()
    oms = [plan7.OptimizedProfile(h, bg, 100) for h in hmms]
    t1 = time.perf_counter()
    plan7._calibrate(oms)
    t2 = time.perf_counter()
    plan7._calibrate(oms)                                              # device images cached
    t3 = time.perf_counter()
    hs = [h.copy() for h in hmms]
    t4 = time.perf_counter()
    for h in hs:
        cal.calibrate(h)
    t5 = time.perf_counter()
    print(f"rep {rep}: profiles {1e3*(t1-t0):.1f} ms | calibrate_batch first {1e3*(t2-t1):.1f} ms = {64/(t2-t1):.0f} /s, "
          f"again (images resident) {1e3*(t3-t2):.1f} ms = {64/(t3-t2):.0f} /s | with profile creation {64/(t2-t0):.0f} /s | "
          f"64 x Calibrator.calibrate (profile + filters + Python fits) {1e3*(t5-t4):.1f} ms = {64/(t5-t4):.0f} /s", flush=True)
