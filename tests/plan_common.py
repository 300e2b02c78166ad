"""What the tests of the work-item plan (sota_imagenet_amd/item_plan.py and the three planners on it) share: the 64-element aligned layout of
the GPU tests' flat buffers, the ResNet-50 fp32 parameter table recorded in tests/golden/flat_layouts.json, and the package's record packer."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def layout(sizes, order=None):
    """64-element aligned offsets of the tensors, laid out in `order`; returns (offsets by tensor, total with a trailing gap)"""
    offs, n = [0] * len(sizes), 0
    for i in (order if order is not None else range(len(sizes))):
        offs[i] = n
        n += (sizes[i] + 63) // 64 * 64
    return offs, n + 64


def resnet50_table():
    """[(name, flat offset, shape)] of the ResNet-50 parameters and the flat array's length, from the recorded layout"""
    with open(os.path.join(HERE, "golden", "flat_layouts.json")) as fh:
        lay = json.load(fh)
    table = lay["tables"][lay["configs"]["resnet50/fp32"]["table"]]
    return [(name, off, tuple(shape)) for name, kind, off, nd, shape in table if kind == 0], lay["configs"]["resnet50/fp32"]["flat_param_elems"]


def resnet50_params():
    """the same table as [(flat offset, numel)]"""
    table, total = resnet50_table()
    return [(off, int(np.prod(shape))) for _, off, shape in table], total


def table(records, dev):
    """16-byte records on the device, through the package's own packer"""
    from sota_imagenet_amd.item_plan import pack_records

    return pack_records(records, dev)
