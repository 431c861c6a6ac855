"""Census of conv1's hand-written instance lists against the table of tests/test_gpu_conv_instances.py (no GPU: the sources are
parsed, the table is imported).  csrc/conv_fwd_k16.hip's K16_CASE(channels, columns per tile, images per workgroup, plain) and
csrc/conv_dw16.hip's DW16_CASE(channels, chunks per row) each stand for a FAST and an EXACT kernel; an instance added to either list
without a FAST row and an EXACT row in that table -- or a cell whose expected route no longer agrees with the lists -- fails here.
The batch-norm instances (DW16_CASE_DENSE, K16_CASE(..., true)) are tests/test_gpu_batchnorm_training.py's: it must name their
channel counts."""
import os
import re

from tests import test_gpu_conv_instances as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cartpoleplusplus_amd", "csrc")
FWD_CLASS = {(1, 4): "<=16", (2, 4): "18..32", (2, 2): "34..64", (2, 1): "66..128"}      # conv_fwd_k16_dispatch: xt = W > 16 ? 2 : 1, ipw by W
DW_CLASSES = {1: ("<=16", "18..32"), 2: ("34..64",), 4: ("66..128",)}                   # conv_dw16_dispatch: nchk = W > 64 ? 4 : (W > 32 ? 2 : 1)


def _calls(name, macro):
    """argument lists of the uses of `macro` in csrc/<name> (its #define and mentions in comments left out)"""
    with open(os.path.join(CSRC, name)) as f:
        text = f.read()
    out = []
    for line in text.splitlines():
        code = line.split("//")[0]
        if code.lstrip().startswith("#define"):
            continue
        for m in re.finditer(r"\b%s\(([^()]*)\)" % macro, code):
            out.append(tuple(a.strip() for a in m.group(1).split(",")))
    return out


def _instances():
    fwd, fwd_plain = [], []
    for cin, xt, ipw, plain in _calls("conv_fwd_k16.hip", "K16_CASE"):
        assert plain in ("false", "true"), plain
        (fwd_plain if plain == "true" else fwd).append((int(cin), FWD_CLASS[(int(xt), int(ipw))]))
    dw = [(int(cin), int(nchk)) for cin, nchk in _calls("conv_dw16.hip", "DW16_CASE")]
    dense = [(int(cin), int(nchk)) for cin, nchk in _calls("conv_dw16.hip", "DW16_CASE_DENSE")]
    return fwd, fwd_plain, dw, dense


def test_the_parser_sees_both_lists():
    fwd, fwd_plain, dw, dense = _instances()
    assert len(fwd) >= 15 and len(fwd_plain) >= 1 and len(dw) >= 11 and len(dense) >= 3, (fwd, fwd_plain, dw, dense)
    assert len(set(fwd)) == len(fwd) and len(set(dw)) == len(dw), "an instance is listed twice"
    assert (18, "34..64") in fwd and (30, "66..128") in fwd and (18, 2) in dw and (30, 4) in dw


def _cells(exact):
    return {(r.channels, r.wclass): r for r in T.TABLE if r.exact == exact and r.B >= 2 and r.shape[:2] == T.CLASS_SHAPE[r.wclass]}


def test_every_instance_has_a_fast_row_and_an_exact_row_on_its_route():
    fwd, _plain, dw, _dense = _instances()
    for exact in (False, True):
        cells = _cells(exact)
        what = "EXACT" if exact else "FAST"
        for channels, wclass in fwd:
            row = cells.get((channels, wclass))
            assert row is not None, "K16_CASE %d channels, %s wide: no %s row in tests/test_gpu_conv_instances.py" % (channels, wclass, what)
            assert row.fwd == T.F16, row
        for channels, nchk in dw:
            for wclass in DW_CLASSES[nchk]:
                row = cells.get((channels, wclass))
                assert row is not None, "DW16_CASE %d channels, %s wide: no %s row in tests/test_gpu_conv_instances.py" % (channels, wclass, what)
                assert row.dw == T.F16, row


def test_every_cell_of_the_table_has_a_row_and_its_routes_are_the_lists():
    fwd, _plain, dw, _dense = _instances()
    dw_cells = set((c, w) for c, nchk in dw for w in DW_CLASSES[nchk])
    cells = _cells(False)
    assert len(T.EXPECTED) * len(T.WIDTH_CLASSES) == 32
    for channels, per_class in T.EXPECTED.items():
        for wclass, cell in zip(T.WIDTH_CLASSES, per_class):
            row = cells.get((channels, wclass))
            assert row is not None, "no row for %d channels, %s wide (%s)" % (channels, wclass, cell)
            assert (row.fwd == T.F16) == ((channels, wclass) in fwd), ("conv1 forward", row)
            assert (row.dw == T.F16) == ((channels, wclass) in dw_cells), ("conv1 dW", row)
            assert "%s/%s" % ("Y" if row.fwd == T.F16 else "N", "Y" if row.dw == T.F16 else "N") == cell
            assert int(row.shape[2] * row.shape[3] * row.shape[4]) == channels
    # a channel count in either list that the table does not know is an instance without any row
    assert set(c for c, _w in fwd) | set(c for c, _n in dw) <= set(T.EXPECTED)
    mixed = set(k for k, r in cells.items() if r.fwd != r.dw)
    assert mixed == set(T.MIXED_CELLS), mixed
    for exact in (False, True):
        assert set(T.MIXED_CELLS) <= set(_cells(exact))
    graphs = [r.graph for r in T.TABLE]
    assert all(a != b for a, b in zip(graphs, graphs[1:])), "graph replay and eager rows alternate down the table"
    assert any(r.B == 1 and r.fwd == T.F32 for r in T.TABLE), "one row at B = 1: conv1 forward on the f32 kernel"


def test_the_batch_norm_instances_belong_to_the_batch_norm_file():
    _fwd, fwd_plain, _dw, dense = _instances()
    with open(os.path.join(ROOT, "tests", "test_gpu_batchnorm_training.py")) as f:
        text = f.read()
    shapes = re.findall(r"\((\d+), (\d+), 3, (\d+), (\d+)\)", text)
    named = set(3 * int(c) * int(r) for _h, _w, c, r in shapes)
    for channels in sorted(set(c for c, _ in dense) | set(c for c, _ in fwd_plain)):
        assert channels in named, "test_gpu_batchnorm_training.py names no shape of %d channels (has %s)" % (channels, sorted(named))
