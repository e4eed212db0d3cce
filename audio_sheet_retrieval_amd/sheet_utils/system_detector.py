"""sheet_utils/system_detector.py: the staff-system U-Net (1 x 512 x 512 tiles).

build_model() describes the graph; the layers themselves are the device kernels behind omr.SegmentationNetwork
(csrc/omr_kernels.hip).  Encoder: four levels of two conv_bn blocks (3x3 'same' conv without bias, flip_filters=True,
BatchNorm, ELU) with 8, 16, 32, 64 channels and a 2x2/2 max-pool after levels 1-3; decoder: three levels of
TransposedConv2D 2x2/2 + BN + ReLU, the encoder skip added, BN, two conv_bn blocks; head: 1x1 conv with bias + sigmoid.
"""

INPUT_SHAPE = [1, 512, 512]
NF0 = 8


class UNet(object):
    """what a SegmentationNetwork needs of the Lasagne graph: its input and output shapes and its parameters"""

    def __init__(self, in_shape):
        self.input_shape = tuple(in_shape)
        self.output_shape = (None, 1) + tuple(in_shape[-2:])

    def param_shapes(self):
        """the 99 parameter arrays in lasagne.layers.get_all_params order"""
        return param_shapes(self.input_shape[0])


def _conv_bn(ci, co):
    return [(co, ci, 3, 3), (co,), (co,), (co,), (co,)]          # W, beta, gamma, mean, inv_std


def param_shapes(in_channels=1, nf0=NF0):
    s = []
    ci = in_channels
    for lv in range(4):
        co = nf0 << lv
        s += _conv_bn(ci, co) + _conv_bn(co, co)
        ci = co
    for lv in (2, 1, 0):
        co = nf0 << lv
        s += [(ci, co, 2, 2)] + [(co,)] * 8 + _conv_bn(co, co) + _conv_bn(co, co)
        ci = co
    s += [(1, nf0, 1, 1), (1,)]
    return s


def build_model(in_shape=INPUT_SHAPE):
    """Compile net architecture"""
    return UNet(in_shape)
