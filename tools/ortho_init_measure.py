"""What profiles/ortho_init.json holds: for every case of tests/test_ortho_init_gpu.py and for the three largest ResNet-50 tensors, the two errors of
mi355_ortho_init (max entry distance to the float64 QR's Q, max |QtQ - I| formed in float64) next to the same two of a float32 QR on the CPU; the
whole-model launch (ResNet-50, 54 matrices) timed once with events, and a few tensors launched alone.  python tools/ortho_init_measure.py --out FILE"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_ortho_init_gpu as T  # noqa: E402
from sota_imagenet_amd import item_plan, ops  # noqa: E402
from sota_imagenet_amd.callbacks import OrthoInitClb  # noqa: E402
from sota_imagenet_amd.fit_wrapper import RunnerState  # noqa: E402
from sota_imagenet_amd.models import resnet50  # noqa: E402

LARGEST = ("layer4.0.conv2.weight", "layer4.0.downsample.0.weight", "fc.weight")
ALONE = LARGEST + ("layer3.0.downsample.0.weight", "layer1.0.conv1.weight", "conv1.weight")


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fields = ("device_dist", "device_defect", "fp32_qr_dist", "fp32_qr_defect")
    out = {"what": __doc__.split("  python")[0].strip(), "cases": [], "model_tensors": [], "alone_ms": {}}
    k = T.run_cases(dev)
    for i, (rows, chans, taps, _) in enumerate(T.CASES):
        Q64, yard = k["refs"][i]
        got = T.errors(T.oriented(T.logical(k["out"], k["recs"][i])), Q64)
        out["cases"].append(dict(rows=rows, chans=chans, taps=taps, **dict(zip(fields, got + yard))))
    m = resnet50(dtype="bf16").cuda()
    cb = OrthoInitClb()
    cb.set_state(RunnerState(model=m))
    cb.fill()
    gauss = m.flat_params.detach().cpu().clone()
    recs = cb.records
    table = item_plan.pack_records(recs, dev, item_plan.ORTHO_FIELDS)
    status = []
    out["whole_model_ms"] = _timed(lambda: status.append(ops.ortho_init_(m.flat_params, recs, table, 1.0)))
    out["whole_model_matrices"], out["whole_model_status_all_zero"] = len(recs), status[0].tolist() == [0] * len(recs)
    after = m.flat_params.detach().cpu()
    for name in ALONE:
        rec = recs[cb.names.index(name)]
        off, rows, chans, taps = rec
        if name in LARGEST:
            A = T.oriented(T.logical(gauss, rec))
            Q64 = T.qr_fixed(A.double())
            got, yard = T.errors(T.oriented(T.logical(after, rec)), Q64), T.errors(T.qr_fixed(A.clone()), Q64)
            out["model_tensors"].append(dict(name=name, rows=rows, chans=chans, taps=taps, **dict(zip(fields, got + yard))))
        m.flat_params[off:off + rows * chans * taps].copy_(gauss[off:off + rows * chans * taps].to(dev))
        one = item_plan.pack_records([rec], dev, item_plan.ORTHO_FIELDS)
        out["alone_ms"][name] = _timed(lambda: ops.ortho_init_(m.flat_params, [rec], one, 1.0))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
