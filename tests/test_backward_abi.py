"""The backward pass at the drop-in boundary, without a GPU: the new names are declared in include/gnnvc.h, bound in engine.py and
exported by the library; null engines are rejected; the ABI version and the block size of the parameter gradients stand."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G
from gnn_mwvc_amd.engine import ABI_SYMBOLS, GRAD_BLOCK_ROWS

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = ["gnnvc_num_params", "gnnvc_get_params", "gnnvc_train_forward", "gnnvc_train_forward_device", "gnnvc_backward",
         "gnnvc_backward_device", "gnnvc_graph_layer_backward", "gnnvc_linear_backward", "gnnvc_relu_backward",
         "gnnvc_sigmoid_backward"]


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_names_are_in_header_and_binding(lib):
    hdr = (ROOT / "include" / "gnnvc.h").read_text()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", hdr, re.M), name
        assert name in ABI_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.gnnvc_abi_version() == 1
    m = re.search(r"#define GNNVC_GRAD_BLOCK_ROWS (\d+)", hdr)
    assert m and int(m.group(1)) == GRAD_BLOCK_ROWS == 4096
    for method in ("num_params", "params", "train_forward", "backward", "graph_layer_backward", "linear_backward", "relu_backward",
                   "sigmoid_backward"):
        assert callable(getattr(G.Engine, method)), method


def test_null_engines_are_rejected(lib):
    n = C.c_uint64(7)
    assert lib.gnnvc_num_params(None, C.byref(n)) == -1 and n.value == 7
    assert lib.gnnvc_get_params(None, None) == -1
    assert lib.gnnvc_train_forward(None, None, None, None) == -1
    assert lib.gnnvc_train_forward_device(None, None, None, None) == -1
    assert lib.gnnvc_backward(None, None, None, None, 0) == -1
    assert lib.gnnvc_backward_device(None, None, None, None, 1) == -1
    assert lib.gnnvc_graph_layer_backward(None, 1, None, None) == -1
    assert lib.gnnvc_linear_backward(None, 1, 1, 1, None, None, None, None, None, None, 0) == -1
    assert lib.gnnvc_relu_backward(None, 1, None, None, None) == -1
    assert lib.gnnvc_sigmoid_backward(None, 1, None, None, None) == -1


def test_no_option_key_was_added():
    """The backward pass is reached through its own calls: gnnvc_set_option's table has no key of it."""
    table = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h").read_text()
    keys = set(re.findall(r'"([a-z_0-9]+)"', table))
    assert keys and not [k for k in keys if "backward" in k or "train" in k or "grad" in k or "symmetric" in k]
