"""The three planners on sota_imagenet_amd/item_plan.py (optim._Layerwise, callbacks.SAMOriginal, callbacks.SAM) pinned byte for byte on the
host: every table they build over the ResNet-50 fp32 layout of tests/golden/flat_layouts.json — 161 tensors in one storage pair and one
param group, in one pair and two groups (ndim > 1 against the rest, train.filter_from_weight_decay's split), and in two pairs (tensor i in
pair i % 2, each pair laid out on its own as the GPU tests do) — hashes to the digest the planners gave before they shared that module."""
import hashlib

import numpy as np
import pytest

from plan_common import layout, resnet50_table
from sota_imagenet_amd import native

# SHA-256 of every table, recorded from the code of commit f225b4d ("Add native SAM callback with per-tensor and per-output-unit norms"), the
# parent of the commit that introduced item_plan.py: SAMOriginal.plan_tables, SAM.plan_tables and SAM._table as they were, and for _Layerwise,
# which had no pure host part then, lines 522-538 of its optim.py (the grouping and the two record tables) with the per-pair and per-group
# ranges of the lines that follow.  A digest that differs means a planner builds another table: the planner is wrong, never the digest.
DIGESTS = {
    "one_pair_one_group": {
        "layerwise": {
            "items": "67933b320dca79270471a27f1c2e1ff25a41ad6c54d80507b1a8c38428e2b900",
            "tensors": "2f8ba34d45e9fc020769f28be3a97eb48a736e9dac3560cc319a563e449abcd8",
            "pairs": "e2a45c1d012f7afd940f0f6c1827300a658ccfa26a41549df5b4bdf36a971cf5",
            "groups": "e54ab40888cd336c5f3e945071a6a851e42f9f4040fe92f8c8ca0ceeffd1307b",
        },
        "sam_original": {
            "items": "67933b320dca79270471a27f1c2e1ff25a41ad6c54d80507b1a8c38428e2b900",
            "kind": "5c1999a68955b466a2e1645b6aaef3d53eb8af6e2ae8fa2940e556c6f647d7ad",
            "pairs": "48e3b7aa3ccb003eebd1fe918e71012dd4aa4d7e2dd64fdf1e9fdbb5e3309ba1",
        },
        "sam_layerwise": {
            "items": "67933b320dca79270471a27f1c2e1ff25a41ad6c54d80507b1a8c38428e2b900",
            "tensors": "c22313638a13c741d4ff5929c98932f85c503b552ddcfa4bb4845ad210243bcc",
            "pieces": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
            "whole": "67933b320dca79270471a27f1c2e1ff25a41ad6c54d80507b1a8c38428e2b900",
            "slots": "fae40447100a366b2cf2e1b86a9d0f10c32b22edc683736dc309119fa503313f",
            "pairs": "696eb42c74abaa1460df335e0171c978767d3efbe7bc9f7fac7df453576cd13c",
        },
        "sam_unitwise": {
            "items": "67933b320dca79270471a27f1c2e1ff25a41ad6c54d80507b1a8c38428e2b900",
            "tensors": "18e9ba120393887f878d0a9a2ce6fd8c3fde61bc6fce295610cdf507f092a2ea",
            "pieces": "d24a5664359bdafd9c978a25c65941841c00b35e1b92f69d53ab516fde459d7c",
            "whole": "6c7a97d20e533ed72e507b5bc62aff6641875efd9ea85ac7b8df962764d00173",
            "slots": "c5492db5f3a983d3de69eb6fce3774255ef7f3e9564f0bebd56fb27080ad4cae",
            "pairs": "362bf7d16fb59ad3571f1c9bcccb23a6453b4b6e8da69cbc225e916b159a8755",
        },
    },
    "one_pair_two_groups": {
        "layerwise": {
            "items": "cdc624164bacfbd21dc64ff43ba16f0fc47cf8da6223f57e048411ef6c1529cf",
            "tensors": "7271970b290b49a30e909b18e519e5cc13227e001090f0b2fbd5ee6ae9900658",
            "pairs": "5d7b0d677c1d16873013797b1d320eb1b7f83b5e71a66cadfa298b95b105c12a",
            "groups": "60e8e0df2659dbb37d4ba41af7941d0a096c8f7b6a3aedcf7dc53171ba931fb2",
        },
        "sam_original": {
            "items": "cdc624164bacfbd21dc64ff43ba16f0fc47cf8da6223f57e048411ef6c1529cf",
            "kind": "0eca95b404af114c83d9eb61180a2ddc6f68bd13702cafa2e67d131b9e02189f",
            "pairs": "48e3b7aa3ccb003eebd1fe918e71012dd4aa4d7e2dd64fdf1e9fdbb5e3309ba1",
        },
        "sam_layerwise": {
            "items": "cdc624164bacfbd21dc64ff43ba16f0fc47cf8da6223f57e048411ef6c1529cf",
            "tensors": "4788288da01800e78749af96985a8e5468e652c6f24aa6590e4b2e1389a62eb7",
            "pieces": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
            "whole": "cdc624164bacfbd21dc64ff43ba16f0fc47cf8da6223f57e048411ef6c1529cf",
            "slots": "b4fe07deea259ab5d2860b9232aef7743f383f2d3b56c795a93af50680285666",
            "pairs": "696eb42c74abaa1460df335e0171c978767d3efbe7bc9f7fac7df453576cd13c",
        },
        "sam_unitwise": {
            "items": "cdc624164bacfbd21dc64ff43ba16f0fc47cf8da6223f57e048411ef6c1529cf",
            "tensors": "2a76b2fb872c0593952445cda1dd553e1b931fdaac02612466d23862d4f49a7d",
            "pieces": "aa8659751a9b984629ab2de198cfef19b479de4394ca5cb4c7d2bb5ba8cb4143",
            "whole": "56f3c60200c8bde8641d76cc32e4861bf1c992e4be354bd51636f5a2352480c8",
            "slots": "2cb99bd5df36e7107aa93f0cfed97bfe32703a6b347fbf0691413a45f07ce8e3",
            "pairs": "362bf7d16fb59ad3571f1c9bcccb23a6453b4b6e8da69cbc225e916b159a8755",
        },
    },
    "two_pairs": {
        "layerwise": {
            "items": "0881311900dfbc896a560f802028ee9a2db5421e939f898810e13b23e1901787",
            "tensors": "4c67f0ee21cd08a0f46910cf5bd7adaadf801b0f6d9d76e4a1a72147f8410794",
            "pairs": "1ae9fd781b2ebf1f97a5e3fa5005b47d5997ca64ea2854d2f9ae8325868149e6",
            "groups": "e54ab40888cd336c5f3e945071a6a851e42f9f4040fe92f8c8ca0ceeffd1307b",
        },
        "sam_original": {
            "items": "0881311900dfbc896a560f802028ee9a2db5421e939f898810e13b23e1901787",
            "kind": "5c1999a68955b466a2e1645b6aaef3d53eb8af6e2ae8fa2940e556c6f647d7ad",
            "pairs": "536b6fcb427863b6b7f390571685e608bd2e91aede7683cd6d563edf5562216c",
        },
        "sam_layerwise": {
            "items": "0881311900dfbc896a560f802028ee9a2db5421e939f898810e13b23e1901787",
            "tensors": "427725114b58b701cd7930fc49c159d9927a7aeebc5f1cfcbcfdfa52d6d24917",
            "pieces": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
            "whole": "0881311900dfbc896a560f802028ee9a2db5421e939f898810e13b23e1901787",
            "slots": "6344e5bcfe07da94401af0a779208f6bad2974578de1ce43d9a553a300a4aea5",
            "pairs": "1a8a56eedccf7419c3a07729e09ba8e3a13fe803b70138c756c7755262c83a7f",
        },
        "sam_unitwise": {
            "items": "0881311900dfbc896a560f802028ee9a2db5421e939f898810e13b23e1901787",
            "tensors": "9399f28e0358f2afdf20de33a0df1056b3ba1fd0566751998e4c283bdecc3638",
            "pieces": "ea5a20264b6a2a8dcc7785fe54a91c2163170c888fcaf7b64a0d8db631e2d012",
            "whole": "7ef95a4e5a09df2c796d6d9619a135033ec47a173fc229766f5d80743efbc98f",
            "slots": "aae2100c8a9df85c6336748cc675ae5fcdb38824a1fc8b292ca6066a331403a5",
            "pairs": "da0e0fd9116977ba0e280b596bf49b6fa484a59781400c2de1a6faea8703e70f",
        },
    },
}

PB, GB, STEP = 1 << 20, 1 << 30, 1 << 28  # stand-ins for the storage addresses: the planners only compare them


def _arrangement(name):
    """[(param base, grad base, first elem, shape, group index)] in param-group order"""
    table, _ = resnet50_table()
    if name == "one_pair_one_group":
        return [(PB, GB, off, shape, 0) for _, off, shape in table]
    if name == "one_pair_two_groups":
        return ([(PB, GB, off, shape, 0) for _, off, shape in table if len(shape) > 1]
                + [(PB, GB, off, shape, 1) for _, off, shape in table if len(shape) <= 1])
    sizes = [int(np.prod(shape)) for _, _, shape in table]
    out = [None] * len(table)
    for b in range(2):
        idx = [i for i in range(len(table)) if i % 2 == b]
        offs, _ = layout([sizes[i] for i in idx])
        for i, o in zip(idx, offs):
            out[i] = (PB + b * STEP, GB + b * STEP, o, table[i][2], 0)
    return out


def _flatten(x):
    if isinstance(x, (list, tuple)):
        return [len(x)] + [v for y in x for v in _flatten(y)]
    return [int(x)]


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _ranges(x):
    """nested ranges and index lists as int64, every list behind its length"""
    return _sha(np.asarray(_flatten(x), dtype=np.int64).tobytes())


def _int32s(x):
    """a table the planners upload as int32"""
    return _sha(np.asarray(x, dtype=np.int32).tobytes())


def _packed(records, **kw):
    """16-byte records: the bytes the device gets"""
    from sota_imagenet_amd.item_plan import pack_records

    return _sha(pack_records(records, **kw).numpy().tobytes())


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_every_table_of_the_three_planners_is_what_it_was(name):
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAM, SAMOriginal
    from sota_imagenet_amd.item_plan import TENSOR_FIELDS

    W = int(native.lib().mi355_lw_item_elems())
    arr = _arrangement(name)
    sizes = [int(np.prod(shape)) for _, _, _, shape, _ in arr]
    assert len(arr) == 161 and len({(pb, gb) for pb, gb, *_ in arr}) == (2 if name == "two_pairs" else 1)
    got = {}
    tab = optim._Layerwise.plan_tables([(pb, gb, off, n, gi) for (pb, gb, off, _, gi), n in zip(arr, sizes)], W)
    got["layerwise"] = dict(items=_packed(tab["items"]), tensors=_packed(tab["tensors"], fields=TENSOR_FIELDS), pairs=_ranges(tab["pairs"]),
                            groups=_ranges(tab["groups"]))
    items, kind, pairs = SAMOriginal.plan_tables([(pb, gb, off, n, len(shape)) for (pb, gb, off, shape, _), n in zip(arr, sizes)], W)
    got["sam_original"] = dict(items=_packed(items), kind=_int32s(kind), pairs=_ranges(pairs))
    for unitwise in (False, True):
        tab = SAM.plan_tables([(pb, gb, off, n, SAM.unit_len(shape, (n // shape[0],) + (1,) * (len(shape) - 1), unitwise))
                               for (pb, gb, off, shape, _), n in zip(arr, sizes)], W)
        got["sam_unitwise" if unitwise else "sam_layerwise"] = dict(
            items=_packed(tab["items"]), tensors=_packed(tab["tensors"]), pieces=_packed(tab["pieces"]), whole=_packed(tab["whole"]),
            slots=_int32s(tab["slots"]), pairs=_ranges(tab["pairs"]))
    for planner, want in DIGESTS[name].items():
        for table, digest in want.items():
            assert got[planner][table] == digest, (name, planner, table)
    assert {p: set(t) for p, t in got.items()} == {p: set(t) for p, t in DIGESTS[name].items()}
