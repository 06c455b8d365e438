"""Training step on MI355X.

What the reference does per step (trainers/ssc.py:57-96, bin/ssc_train.py:331-359): `Serenade.forward` -> cfm_loss +
prior_loss -> `backward()` -> DDP gradient all-reduce over NCCL -> `clip_grad_norm_(1.0)` -> AdamW(lr 8e-4).  Here:

  * `TrainSerenade`  the whole model (serenade.py:35-166) for training: every trainable tensor of the checkpoint under
                     its reference name, all views of ONE flat fp32 buffer (and one flat gradient buffer);
  * `Estimator`      the flow-matching decoder (matcha_components/decoder.py, 192 tensors, >99 % of the FLOPs): forward
                     over the same channels-last HIP kernels as inference, every op an autograd node whose backward is
                     HIP again; `cfm_loss` = flow_matching.py:95-133 around it;
  * `GradSync`       the DDP replacement: the flat gradient buffer is all-reduced over RCCL in buckets that are
                     launched from backward hooks as soon as their parameters are done (overlaps the rest of backward);
  * `AdamW`          clip_grad_norm_ + torch.optim.AdamW as one fused kernel launch over the flat buffers (srn_adamw).

Division of labour.  GEMM-shaped gradients that contract over channels -- dgrad of every conv / projection (a conv of
dY with the tap-reversed, transposed weights), dP = dO V^T and dQ = dS K of attention -- are `srn_conv_gemm` launches;
row / column reductions and activations (GroupNorm+Mish, LayerNorm / SpeakerAdapter, softmax, GEGLU) are the kernels of
csrc/train.hip.  Gradients that contract over TIME (wgrad = dY^T X, dV = P^T dO, dK = dS^T Q) are transposed-A GEMMs
and are `srn_tn_gemm` launches (ops.TnGemmOp).  torch autograd is the tape; mask multiplies, concatenations,
LeakyReLU / dropout, weight-norm folding, the (B, 2048) time-embedding activations and the scalar loss reductions are
torch ops on the same device.  The GST style encoder (0.8 GFLOP of a ~1.3 TFLOP step: 3x3 Conv2d + train-mode
BatchNorm2d, a 16-step GRU, 50-token attention) runs on the same contractions plus the srn_bn_relu_*, srn_gru_train_*
and srn_token_attn_* kernels in both directions (`TrainSerenade.gst`).  Dropout uses
torch's generator (the reference's draws cannot be reproduced); parity tests run with dropout off against the
reference's own gradients (tests/golden/train_grads_L45.npz, train_full_T64.npz).

Modules: `functions` the autograd nodes over the kernels, `model` the parameter store and the training model, `optim`
gradient all-reduce / optimizer / schedule / checkpoints, `graphed` the captured step.  Launches are built by the
builders the inference plans use (plan.conv_op, plan.attention_ops, the ops.*Op classes, ops.call).
"""
from ..plan import require_cuda as _require_cuda  # the package's one binding: the submodules call it through here
from .functions import NORM_BWD_ROWS, attention_core, conv1d, geglu, gn_mish, pack_conv, row_ln  # noqa: F401
from .graphed import GraphedStep, count_memset_nodes  # noqa: F401
from .model import Estimator, ParamStore, TrainSerenade, cfm_loss
from .optim import AdamW, GradSync, MultiStepLR, load_checkpoint, save_checkpoint

__all__ = ["Estimator", "TrainSerenade", "ParamStore", "GraphedStep", "MultiStepLR", "save_checkpoint", "load_checkpoint", "GradSync", "AdamW", "cfm_loss", "conv1d", "gn_mish", "row_ln", "attention_core", "geglu"]
