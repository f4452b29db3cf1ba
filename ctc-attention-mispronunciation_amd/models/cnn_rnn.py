"""Drop-in for the reference's CTC-only baseline ``models/cnn_rnn.py`` (CRC/models/cnn_rnn.py): the acoustic model of
``models/model_ctc.py`` without the text encoder and the attention.

Same class names, constructor arguments, ``state_dict`` keys (45 float entries at 4 layers: ``conv.*``, ``rnns.*``, ``fc.0.*`` [2H],
``fc.1.weight`` [C, 2H]), ``forward(x, x1[, visualize])`` signature -- ``x1`` is accepted and ignored, as the reference ignores it
(cnn_rnn.py:147) -- and return layout ([T/2, B, C] log-probabilities).  The containers and the library plumbing are those of
``models.model_ctc``; the eval forward runs behind a handle of mdd_create_ctc (include/mdd_hip.h).  Training this model is not built:
``forward`` in train mode raises NotImplementedError.
"""
import math  # noqa: F401  (re-exported, as models.model_ctc does)

import torch  # noqa: F401
import torch.nn as nn  # noqa: F401
import torch.nn.functional as F  # noqa: F401

from . import model_ctc
from .model_ctc import BatchRNN, LayerCNN, ed  # noqa: F401  (the names the reference module exposes through ``import *``)


class CTC_Model(model_ctc.CTC_Model):
    _ctc_only = True
