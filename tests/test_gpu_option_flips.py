"""Options flipped between forwards on a resident graph of the trained shape (tools/optionflips.py's cases, tests/flip_harness.py's
checks; tests/test_option_flips_inputs.py pins the table and shows on the CPU that every case moves its key across its graph).

include/gnnvc.h gives gnnvc_set_option's keys one line of contract, "take effect at the next graph upload / attach"; many are read
inside every forward.  What holds for all of them, and is held here: whenever a key is set, under whatever plans are in force, every
forward and stage call that follows gives the oracle's bits; a graph handed over afterwards leaves the engine in the state of a
fresh one with the same options; a key flipped back leaves no trace.

  test_directed            one test per key of gnnvc_options.h's table (but tools/optionflips.EXCLUDED): every value of its domain under
                           the graph of tests/test_modelgen.py::GRAPHS where it matters
  test_random_sequences    24 sequences of 12 to 20 steps — sets, forwards, stage calls, the same graph again, graphs of other
                           classes, the weight scale, the stream — in blocks of six
  test_behind_one_handle   the keys a multi-device handle hands on that touch row classes or queues, on three parts (all on device 0)
                           and on a single engine with the same set calls
  test_weight_scale_under_the_lds_table   gnnvc_set_weight_scale under a resident graph whose stage 0 runs on the LDS table: across
                           the table's entry widths and back, the same graph again after every move

Bars: tests/flip_harness.py's, which are the suite's — bit for bit, scores within 1 ulp of the oracle's."""
import pytest

from tools import optionflips as of
from tests import flip_harness as fh
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

KEYS = sorted(of.covered_keys())


@pytest.mark.parametrize("key", KEYS)
def test_directed(shim, key):
    cases = [of.case(i) for i in of.directed_indices() if of.case(i).key == key]
    assert cases
    fh.prepare(cases)
    for c in cases:
        fh.run_case(c, shim)


@pytest.mark.parametrize("block", range(of.N_RANDOM // 6))
def test_random_sequences(shim, block):
    cases = [of.case(i) for i in of.random_indices()[block * 6: block * 6 + 6]]
    fh.prepare(cases)
    for c in cases:
        fh.run_case(c, shim)


@pytest.mark.parametrize("key", of.MULTI)
def test_behind_one_handle(shim, key):
    (c,) = [of.case(i) for i in of.multi_indices() if of.case(i).key == key]
    fh.prepare([c])
    fh.run_multi(c, shim)


@pytest.mark.parametrize("i", of.scale_indices())
def test_weight_scale_under_the_lds_table(shim, i):
    c = of.case(i)
    fh.prepare([c])
    fh.run_case(c, shim)
