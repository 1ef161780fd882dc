"""Error behaviour of the C ABI (include/jaicov_neq.h): what jaicov_neq_create rejects and what the call-order state machine refuses.

The reference throws from the constructor / from estimateModel for the same situations (IllegalArgumentException for malformed models,
e.g. ZernikeDistortionModel.java:67-68 for an order outside 1..119, TangentialDistortionModel owning Bx AND By; IllegalStateException-like
misuse cannot happen there because one method runs the whole loop, BA:203-387).  Here every rejection is a status code
(JAICOV_ERR_BAD_ARGUMENT -1, BAD_STATE -2) plus a text from jaicov_neq_last_error; nothing is repaired silently and no call crashes."""
import dataclasses

import numpy as np
import pytest

from bundle_adjustment_amd import engine
from helpers import base_scene, corrupt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("what", ["datum_flags", "dist_order_of_kinds", "unknown_kind", "zernike_order_0", "zernike_order_120", "not_image_major",
                                  "duplicate_column", "column_out_of_range", "block_spans_images", "blocks_descending", "too_many_coefficients"])
def test_create_rejects_a_malformed_problem(what):
    fp = base_scene()
    engine.Engine(fp).close()                                                            # the scene itself is fine
    bad, text = corrupt(fp, what)
    with pytest.raises(engine.EngineError) as ei:
        engine.Engine(bad)
    assert ei.value.code == (-3 if what == "too_many_coefficients" else -1), str(ei.value)
    assert text in str(ei.value), str(ei.value)


@pytest.mark.parametrize("rng", [(3, 2), (5, 7), (0, 7)])
def test_create_rejects_a_bad_image_range(rng):
    fp = base_scene()
    with pytest.raises(engine.EngineError) as ei:
        engine.Engine(fp, image_range=rng)
    assert ei.value.code == -1 and "image range" in str(ei.value)


def test_create_rejects_an_image_index_out_of_range_on_every_path():
    """Checked for every description, not only where ordinary images may be served as blocks."""
    fp = base_scene()
    im = fp.ip_image.copy(); im[-1] = fp.n_images
    with pytest.raises(engine.EngineError) as ei:
        engine.Engine(dataclasses.replace(fp, ip_image=im), ordinary_group_elimination=-1)
    assert ei.value.code == -1 and "image index out of range" in str(ei.value)


def test_create_rejects_an_unknown_assembly_mode():
    with pytest.raises(engine.EngineError) as ei:
        engine.Engine(base_scene(), assembly_mode=3)
    assert ei.value.code == -1 and "assembly_mode must be" in str(ei.value)


def test_call_order_is_enforced():
    """set_parameters -> (accumulate -> finalize | build) -> solve -> omega / update / results; anything else is JAICOV_ERR_BAD_STATE and leaves
    the engine usable."""
    fp = base_scene()
    s2 = fp.sigma2apriori
    eng = engine.Engine(fp)

    def refused(call, text, code=-2):
        with pytest.raises(engine.EngineError) as ei:
            call()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    refused(lambda: eng.build(s2, 0.0), "set_parameters first")
    refused(lambda: eng.omega(s2, np.zeros(fp.n_unknowns)), "set_parameters first")
    eng.set_parameters(fp.values)
    refused(lambda: eng.solve(False), "build first")
    refused(lambda: eng.finalize(s2, 0.0), "accumulate first")
    refused(lambda: eng.reduce_buffer(), "accumulate first")
    refused(lambda: eng.get_normal(), "build first")
    refused(lambda: eng.build(0.0, 0.0), "variance of unit weight", code=-1)
    refused(lambda: eng.build(-1.0, 0.0), "variance of unit weight", code=-1)
    refused(lambda: eng.get_cofactor_sub(np.arange(3)), "no cofactor matrix")
    assert eng.cofactor_order() == -1
    refused(lambda: eng.eo_step_buffer(), "solve a reduced system first")
    eng.build(s2, 0.0)
    refused(lambda: eng.expansion_buffer(), "expansion buffer")                           # not announced, and already finalized
    refused(lambda: eng.solve(7), "", code=-1)                                            # no such MatrixInversion
    refused(lambda: eng.solve(engine.INVERT_FULL), "prepare_inverse")                     # EO blocks pre-eliminated: FULL must be announced
    dx = eng.solve(False)
    refused(lambda: eng.solve(False), "build first")                                      # one solve per build
    refused(lambda: eng.get_cofactor(), "no cofactor matrix")
    # a wrong buffer length for the cofactor matrix
    eng.prepare_inverse(engine.INVERT_REDUCED)
    eng.build(s2, 0.0)
    eng.solve(engine.INVERT_REDUCED)
    k = eng.cofactor_order()
    assert k == eng.reduced_order()
    Q = np.zeros(k * (k + 1) // 2 + 1)
    rc = eng.L.jaicov_neq_get_cofactor(eng._h, Q.ctypes.data_as(engine.C.POINTER(engine.C.c_double)), Q.size)
    assert rc == -1 and "order(order+1)/2" in eng.L.jaicov_neq_last_error(eng._h).decode()
    # ... and after all the refusals the engine still does its job
    eng.prepare_inverse(engine.INVERT_NONE)
    eng.build(s2, 0.0)
    np.testing.assert_array_equal(eng.solve(False), dx)
    eng.close()


def test_null_handles_and_pointers_are_refused_not_dereferenced():
    L = engine.load_library()
    C = engine.C
    null = C.c_void_p()
    assert L.jaicov_neq_build(null, 1.0, 0.0, 0) == -1
    assert L.jaicov_neq_solve(null, 0, None) == -1
    assert L.jaicov_neq_finalize(null, 1.0, 0.0, 0) == -1
    assert L.jaicov_neq_cofactor_order(null) == -1 and L.jaicov_neq_reduced_order(null) == -1
    fp = base_scene()
    eng = engine.Engine(fp)
    eng.set_parameters(fp.values)
    eng.build(fp.sigma2apriori, 0.0)
    assert L.jaicov_neq_solve(eng._h, 0, None) == -1                                       # no output array
    assert L.jaicov_neq_reduce_buffer(eng._h, None, None) == -1
    eng.close()
