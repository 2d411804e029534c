"""CPU: UNSUPNET.MODEL_TYPE resolves to its loss pair when the model is built; an unknown value raises."""
import pytest


def test_model_type_resolves_to_its_loss_pair():
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.modeling.box_regression import uncertainty_losses
    assert uncertainty_losses("GUASSIAN") == (ops.gaussian_nll_sum, ops.kl_efl_loss)
    assert uncertainty_losses("LAPLACE") == (ops.laplace_nll_sum, ops.laplace_kl_efl_loss)


@pytest.mark.parametrize("model_type", ["GAUSSIAN", "laplace", "", "SMOOTH_L1"])
def test_unknown_model_type_raises(model_type):
    from probabilisticteacher_amd.modeling.box_regression import uncertainty_losses
    with pytest.raises(ValueError, match="MODEL_TYPE"):
        uncertainty_losses(model_type)


@pytest.mark.parametrize("model_type", ["GUASSIAN", "LAPLACE", "GAUSSIAN"])
def test_build_model_honours_model_type(model_type):
    from probabilisticteacher_amd import modeling, ops
    from probabilisticteacher_amd.config import setup_cfg
    cfg = setup_cfg("configs/pt/final_c2f.yaml", ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", "",
                                                   "UNSUPNET.MODEL_TYPE", model_type])
    if model_type == "GAUSSIAN":
        with pytest.raises(ValueError, match="MODEL_TYPE"):
            modeling.build_model(cfg)
        return
    model = modeling.build_model(cfg)
    nll = ops.laplace_nll_sum if model_type == "LAPLACE" else ops.gaussian_nll_sum
    kl = ops.laplace_kl_efl_loss if model_type == "LAPLACE" else ops.kl_efl_loss
    assert model.proposal_generator.nll_loss is nll and model.proposal_generator.kl_loss is kl
    assert model.roi_heads.box_predictor.nll_loss is nll and model.roi_heads.box_predictor.kl_loss is kl
