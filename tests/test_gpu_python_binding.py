"""runtime's argument front on the device: a theta the kernels could not read is refused by every entry point before
anything is launched, every accepted form of the same theta gives the same bits, and a pitched output keeps its padding.
Two subjects with one bolus and three observations each, one_compartment (theta = [ke, v]), three support points."""
import numpy as np
import pytest
import torch

from pharmsol_amd import AssayErrorModel, AssayErrorModels, Data, ErrorPoly, Subject, _ffi, runtime
from tests import models

pytestmark = pytest.mark.gpu

EM = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))
THETA = np.array([[0.10, 10.0], [0.25, 14.0], [0.40, 21.0]])
STATE = {}


def case():
    """(model, device population, contiguous CUDA theta, its predictions, its log-likelihoods), computed once"""
    if not STATE:
        subs = [Subject.builder(f"s{i}").bolus(0.0, 100.0 + 50.0 * i, 0).observation(1.0, 6.0, 0).observation(2.5, 4.0 + i, 0)
                .observation(6.0, 2.0, 0).build() for i in range(2)]
        m = models.handwritten_analytical("one_compartment", 0, 2).with_ndrugs(1)
        pop = runtime.DevicePopulation(m.flatten(Data(subs)), 0)
        assert (pop.n_subjects, pop.n_observations) == (2, 6)
        theta = torch.as_tensor(THETA, device="cuda:0")
        pred, st = runtime.predict(m, pop, theta)
        ll, st_ll = runtime.loglik(m, pop, EM, theta)
        torch.cuda.synchronize()
        assert not st.any() and not st_ll.any() and torch.isfinite(pred).all() and torch.isfinite(ll).all()
        STATE["case"] = (m, pop, theta, pred.cpu().numpy(), ll.cpu().numpy())
    return STATE["case"]


def test_a_theta_the_kernels_cannot_read_is_refused_before_any_launch(monkeypatch):
    m, pop, theta, _, _ = case()

    def lib():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_ffi, "lib", lib)  # every launch goes through it
    wide = torch.cat([theta, theta[:, :1]], dim=1)
    for bad in (theta.to(torch.float32), wide):
        for call in (lambda: runtime.predict(m, pop, bad), lambda: runtime.loglik(m, pop, EM, bad),
                     lambda: runtime.predict_states(m, pop, bad), lambda: runtime.place_predictions(m, pop, bad, search_gib=0.25),
                     lambda: runtime.alloc_predictions(m, pop, bad, tries=1)):
            with pytest.raises(ValueError, match="theta"):
                call()


def test_every_accepted_form_of_theta_gives_the_same_bits():
    m, pop, theta, pred0, ll0 = case()
    transposed = theta.t().contiguous().t()  # a [P, nparams] view of a [nparams, P] tensor
    assert not transposed.is_contiguous() and torch.equal(transposed, theta)
    for form in (transposed, THETA):
        pred, _ = runtime.predict(m, pop, form)
        ll, _ = runtime.loglik(m, pop, EM, form)
        torch.cuda.synchronize()
        assert pred.cpu().numpy().tobytes() == pred0.tobytes() and ll.cpu().numpy().tobytes() == ll0.tobytes()


def test_a_pitched_prediction_buffer_keeps_its_padding():
    m, pop, theta, pred0, _ = case()
    ld = runtime.recommended_ld(3)
    assert ld > 3
    buf = torch.full((pop.n_observations, ld), -7.0, dtype=torch.float64, device="cuda:0")
    pred, _ = runtime.predict(m, pop, theta, pred=buf[:, :3])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert pred.data_ptr() == buf.data_ptr() and got[:, :3].tobytes() == pred0.tobytes() and (got[:, 3:] == -7.0).all()
