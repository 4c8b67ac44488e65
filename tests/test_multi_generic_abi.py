"""CPU-side checks of gnnvc_create_multi_generic (generic-stage models on several devices behind one handle, opt-in at creation)
and gnnvc_push_rows (full rows to every peer in one launch): the header declares both calls and the config struct, the library
exports them, the binding lists and types them and has the parameter and the method, arguments that can be refused without a
device are refused before one is touched, the documents name the call and GNNVC_GENERIC, and the ABI version has not moved.
No compute calls here (tests/test_gpu_multi_generic.py has those)."""
import ctypes as C
import inspect
import pathlib
import re

import pytest

import gnn_mwvc_amd as G
from gnn_mwvc_amd.engine import GenericConfig

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

CREATE = "gnnvc_create_multi_generic"
PUSH = "gnnvc_push_rows"
CREATE_PROTOTYPE = (r"int gnnvc_create_multi_generic\(gnnvc_engine \*\*out, const char \*model_text, size_t len,\s*"
                    r"const int \*devices, int n_devices, const gnnvc_generic_config \*cfg[^)]*\);")
PUSH_PROTOTYPE = (r"int gnnvc_push_rows\(gnnvc_engine \*e, const float \*d_src, uint64_t words, uint32_t n_dst, float \*const \*d_dst, "
                  r"void \*hip_stream\);")
FIELDS = [("uint32_t", "size"), ("uint32_t", "heavy_rows"), ("uint32_t", "giant_rows"), ("int32_t", "giant_segments"),
          ("uint32_t", "big_stages_lds"), ("uint32_t", "feature_width"), ("uint32_t", "patterns")]
ERR_INVALID = -1
MODEL = b"m\n0 Layers\n"


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_header_declares_the_creation_call_next_to_create_multi():
    assert re.search(CREATE_PROTOTYPE, HEADER), f"{CREATE} is not declared with the agreed signature"
    multi = HEADER.index("int gnnvc_create_multi(gnnvc_engine **out")
    mine = HEADER.index("int gnnvc_create_multi_generic(gnnvc_engine **out")
    assert multi < mine < HEADER.index("int gnnvc_set_weight_scale(")
    assert not re.search(r"^int gnnvc_", HEADER[multi + 10: mine], flags=re.M), "another entry point stands between the two"


def test_header_declares_the_struct_and_its_default():
    body = re.search(r"typedef struct gnnvc_generic_config \{(.*?)\} gnnvc_generic_config;", HEADER, flags=re.S)
    assert body, "the config struct is not declared"
    fields = re.findall(r"^\s*(u?int32_t)\s+(\w+);", body.group(1), flags=re.M)
    assert fields == FIELDS
    assert re.search(r"^#define GNNVC_GENERIC_DEFAULT 0xFFFFFFFFu?$", HEADER, flags=re.M)
    assert G.engine.GENERIC_DEFAULT == 0xFFFFFFFF


def test_header_declares_push_rows_beside_push_piece():
    assert re.search(PUSH_PROTOTYPE, HEADER), f"{PUSH} is not declared with the agreed signature"
    piece = HEADER.index("int gnnvc_push_piece(gnnvc_engine *e")
    mine = HEADER.index("int gnnvc_push_rows(gnnvc_engine *e")
    assert piece < mine < HEADER.index("int gnnvc_stage_input_ready(")
    doc = HEADER[HEADER.index("int gnnvc_unpack_pieces(gnnvc_engine *e"): mine]
    for word in ("k_push_rows", "n_dst <= 64", "hip_stream", "NULL", "16-byte", "4-byte", "GNNVC_ERR_INVALID", "Asynchronous"):
        assert word in doc, word


def test_the_comment_in_front_of_the_creation_call_is_its_own():
    doc = HEADER[HEADER.index("int gnnvc_create_multi(gnnvc_engine **out"): HEADER.index("int gnnvc_create_multi_generic(gnnvc_engine **out")]
    for word in ("GNNVC_ERR_INVALID", "GNNVC_ERR_UNSUPPORTED", "any device is touched","gnnvc_set_generic_heavy_rows",
                 "gnnvc_set_generic_giant_rows", "gnnvc_set_generic_big_stages", "gnnvc_set_generic_feature_width",
                 "gnnvc_set_generic_patterns", "gnnvc_push_rows", "gnnvc_stage_forward_device", "gnnvc_audit_stage_device",
                 '"multi_generic"', '"multi_exchanges"', '"multi_exchange_bytes_per_peer_stage<s>"', '"multi_pieces"', '"multi_push"',
                 '"multi_only_part"', '"poison_features"', '"multi_pack"', '"multi_announce"', '"audit_period"', '"audit_repair"'):
        assert word in doc, word


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


def test_library_exports_both_calls_and_the_binding_types_them(lib):
    for name in (CREATE, PUSH):
        assert name in G.engine.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert fn is not None and fn.restype is C.c_int
    vp = C.c_void_p
    assert list(lib.gnnvc_create_multi_generic.argtypes) == [C.POINTER(vp), C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.c_int,
                                                             C.POINTER(GenericConfig)]
    assert list(lib.gnnvc_push_rows.argtypes) == [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(vp), vp]


def test_the_binding_struct_is_the_header_struct():
    kinds = {"uint32_t": C.c_uint32, "int32_t": C.c_int32}
    assert [(name, kind) for name, kind in GenericConfig._fields_] == [(name, kinds[t]) for t, name in FIELDS]
    assert C.sizeof(GenericConfig) == 28
    c = GenericConfig.of()
    assert (c.size, c.heavy_rows, c.giant_rows, c.giant_segments, c.big_stages_lds, c.feature_width, c.patterns) == \
        (28, 0xFFFFFFFF, 0xFFFFFFFF, -1, 0, 0, 0)
    c = GenericConfig.of({"heavy_rows": 0, "patterns": 3})
    assert (c.heavy_rows, c.giant_rows, c.patterns) == (0, 0xFFFFFFFF, 3)
    with pytest.raises(ValueError):
        GenericConfig.of({"heavy": 1})


def _create(lib, cfg, out=True, model=MODEL, devices=(0, 0)):
    h = C.c_void_p(0xDEAD)   # (a refusal leaves null behind, whatever stood there)
    arr = (C.c_int * len(devices))(*devices)
    rc = lib.gnnvc_create_multi_generic(C.byref(h) if out else None, model, len(model) if model else 0, arr, len(devices),
                                        C.byref(cfg) if cfg is not None else None)
    return rc, h.value


def test_arguments_are_refused_before_any_device_is_touched(lib):
    """Each of these is GNNVC_ERR_INVALID with *out null — on a machine without a GPU too, where touching a device would have
    answered GNNVC_ERR_DEVICE instead."""
    assert _create(lib, GenericConfig.of(), out=False)[0] == ERR_INVALID
    assert _create(lib, GenericConfig.of(), model=None) == (ERR_INVALID, None)
    for off in (-4, 4):
        c = GenericConfig.of()
        c.size += off
        assert _create(lib, c) == (ERR_INVALID, None), off
    assert _create(lib, GenericConfig.of({"patterns": 4})) == (ERR_INVALID, None)
    assert _create(lib, GenericConfig.of({"feature_width": 65})) == (ERR_INVALID, None)
    # the other values the single-device setters reject
    assert _create(lib, GenericConfig.of({"feature_width": 32})) == (ERR_INVALID, None)
    assert _create(lib, GenericConfig.of({"big_stages_lds": 65535})) == (ERR_INVALID, None)
    assert _create(lib, GenericConfig.of({"big_stages_lds": 163841})) == (ERR_INVALID, None)
    h = C.c_void_p(0xDEAD)
    assert lib.gnnvc_create_multi_generic(C.byref(h), MODEL, len(MODEL), None, 2, None) == ERR_INVALID and not h.value
    assert _create(lib, None, devices=()) == (ERR_INVALID, None)


def test_push_rows_refuses_a_null_engine(lib):
    assert lib.gnnvc_push_rows(None, None, 0, 0, None, None) == ERR_INVALID


def test_binding_has_the_parameter_and_the_method():
    sig = inspect.signature(G.Engine.__init__)
    assert "generic" in sig.parameters and sig.parameters["generic"].default is None
    assert CREATE in G.Engine.__init__.__doc__
    for key in GenericConfig.KEYS:
        assert key in G.Engine.__init__.__doc__, key
    fn = getattr(G.Engine, "push_rows", None)
    assert callable(fn) and PUSH in fn.__doc__ and "k_push_rows" in fn.__doc__
    with pytest.raises(ValueError):
        G.Engine("m\n0 Layers\n", generic=True)   # (refused before the library is asked: generic= goes with devices=)


def test_the_option_table_is_not_where_it_lives():
    table = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h").read_text()
    assert "multi_generic" not in table and "multi_exchanges" not in table


@pytest.mark.parametrize("doc", ["INTEGRATION.md", "README.md", "DESIGN.md"])
def test_the_documents_name_the_call(doc):
    assert CREATE in (ROOT / doc).read_text(), doc


def test_the_documents_name_the_environment_variable_and_the_kernel():
    assert "GNNVC_GENERIC" in (ROOT / "INTEGRATION.md").read_text()
    assert "GNNVC_GENERIC" in (ROOT / "gnn-mwvc_amd" / "host" / "gnn_inference.cpp").read_text()
    design = (ROOT / "DESIGN.md").read_text()
    assert "k_push_rows" in design and "forward_part_generic" in design
    assert "k_push_rows" in (ROOT / "profiles" / "generic_stages" / "README.md").read_text()
