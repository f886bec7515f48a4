"""CPU-side checks of the Predictor class structure (pnpp_hip/inference.py, pointnet_inference.py, transformer_inference.py): the
base class is every family's base and their factory, no class carries a method of another family, every family refuses a CPU model
with the one error, and planes_to_float32 is the documented view of a blob's three fragment-major bf16 planes.  No GPU, no library
call."""
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)


def _classes():
    from pnpp_hip.inference import ClsPredictor, Predictor, SetAbstractionPredictor
    from pnpp_hip.pointnet_inference import PointNetPredictor
    from pnpp_hip.transformer_inference import TransformerPredictor
    return Predictor, SetAbstractionPredictor, ClsPredictor, PointNetPredictor, TransformerPredictor


def test_subclass_relations():
    Predictor, SetAbstractionPredictor, ClsPredictor, PointNetPredictor, TransformerPredictor = _classes()
    assert issubclass(SetAbstractionPredictor, Predictor) and SetAbstractionPredictor is not Predictor
    assert issubclass(ClsPredictor, SetAbstractionPredictor)
    assert issubclass(PointNetPredictor, Predictor) and not issubclass(PointNetPredictor, SetAbstractionPredictor)
    assert issubclass(TransformerPredictor, Predictor) and not issubclass(TransformerPredictor, SetAbstractionPredictor)


def test_no_class_carries_another_family_s_methods():
    _, _, _, PointNetPredictor, TransformerPredictor = _classes()
    assert not hasattr(TransformerPredictor, "_level")
    assert not hasattr(TransformerPredictor, "folded_layer")
    assert not hasattr(PointNetPredictor, "_levels12")


def _cpu_models():
    from models.point_transformer import PointTransformer
    from models.pointnet import PointNet
    from models.pointnet_pp_cls import PointNetPlusPlusCls
    from models.pointnet_pp_vonMises import PointNetPPVonMises
    return {"set-abstraction": PointNetPPVonMises, "classifier": PointNetPlusPlusCls, "pointnet": lambda: PointNet(True),
            "transformer": lambda: PointTransformer(depth=2)}


@pytest.mark.parametrize("family", ["set-abstraction", "classifier", "pointnet", "transformer"])
def test_predictor_of_a_cpu_model_has_no_cpu_fallback(family):
    from pnpp_hip import Predictor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Predictor(_cpu_models()[family]())


def test_predictor_of_an_unknown_model_is_a_type_error():
    from pnpp_hip import Predictor
    with pytest.raises(TypeError, match="Predictor takes a PointNet\\+\\+ set-abstraction model, a PointNetPlusPlusCls, a PointNet, "
                                        "a PointNetEncoder or a PointTransformer, not object"):
        Predictor(object())


def _blob_of(m: torch.Tensor, offset: int) -> torch.Tensor:
    """a uint8 blob holding, `offset` bytes in, the three bf16 planes of the float32 matrix m: high, middle and low parts by repeated
    rounding, each plane fragment-major [rows/32][ld/16][2][32][8] with rows n = 32 cb + r and columns k = 16 ks + 8 h + j"""
    rows, ld = m.shape
    parts, rest = [], m.clone()
    for _ in range(3):
        parts.append(rest.bfloat16())
        rest = rest - parts[-1].float()
    assert float(rest.abs().max()) == 0.0, "the matrix is not the sum of three bf16 parts"
    planes = torch.zeros(3 * rows * ld, dtype=torch.bfloat16)
    for p, part in enumerate(parts):
        for n in range(rows):
            for k in range(ld):
                cb, r, ks, h, j = n // 32, n % 32, k // 16, (k % 16) // 8, k % 8
                planes[((((p * (rows // 32) + cb) * (ld // 16) + ks) * 2 + h) * 32 + r) * 8 + j] = part[n, k]
    blob = torch.full((offset + 6 * rows * ld + 16,), 0xA5, dtype=torch.uint8)   # neighbours that are no zeros
    blob[offset:offset + 6 * rows * ld] = planes.view(torch.uint8)
    return blob


@pytest.mark.parametrize("rows,ld,offset", [(32, 16, 0), (64, 32, 0), (64, 32, 256)], ids=["one-fragment", "2x2-blocks", "offset"])
def test_planes_to_float32_is_the_fragment_major_view(rows, ld, offset):
    from pnpp_hip.inference import planes_to_float32
    m = torch.randn(rows, ld, generator=torch.Generator().manual_seed(rows + ld)) * 3.0
    got = planes_to_float32(_blob_of(m, offset), offset, rows, ld)
    assert got.dtype == torch.float32 and got.shape == (rows, ld)
    assert torch.equal(got, m)
