"""MI355X-native Vec2Wav generator forward (the hot path of p1an-lin-jung/WavThruVec_pytorch).

Public surface = the reference's: `Generator`, `ResBlock1`, `ResBlock2`, `ConditionalBatchNorm1d`,
`get_padding`, `init_weights`, `hparams`; `AdamW` (optim.py) is torch.optim.AdamW stepping in one launch of the library, with global-norm
clipping and a non-finite guard that stay on the GPU; `clip_grad_norm_` is the stand-alone clip; `AdamW(ema_decay=)` keeps an
exponential moving average of the weights in the step's own launch and `ema_state_dict` writes its checkpoint; `resample` and
`peak_normalize` (audio.py) are the sample-rate conversion and peak normalisation at the two ends of the audio path.  Importing the package does not touch the GPU or load the HIP
library; the first `Generator.forward` does, and raises if the library is missing.
"""
from .models import Generator, ResBlock1, ResBlock2, LRELU_SLOPE  # noqa: F401
from .modules import ConditionalBatchNorm1d  # noqa: F401
from .utils import get_padding, init_weights  # noqa: F401
from . import hparams  # noqa: F401
from .optim import AdamW, clip_grad_norm_, ema_state_dict  # noqa: F401
from . import stft_loss  # noqa: F401  (the module: stft_loss.stft_loss is the one-resolution function)
from .stft_loss import MultiResolutionSTFTLoss  # noqa: F401
from . import audio  # noqa: F401
from .audio import resample, resample_table, resampled_length, peak_normalize, mask_tail  # noqa: F401
from .mel import mel_loss  # noqa: F401  (the mel L1 training loss in one call, with or without per-item lengths)

__all__ = ['Generator', 'ResBlock1', 'ResBlock2', 'ConditionalBatchNorm1d', 'get_padding', 'init_weights',
           'hparams', 'LRELU_SLOPE', 'AdamW', 'clip_grad_norm_', 'ema_state_dict', 'MultiResolutionSTFTLoss', 'stft_loss',
           'audio', 'resample', 'resample_table', 'resampled_length', 'peak_normalize', 'mask_tail', 'mel_loss']
