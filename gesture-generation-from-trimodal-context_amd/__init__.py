"""MI355X-native (gfx950) implementation of the trimodal gesture-generation GAN hot path.

Drop-in for the reference's PoseGenerator / ConvDiscriminator / pose-mode EmbeddingNet nn.Modules and its
train_iter_gan step; all arithmetic runs in hand-written HIP kernels (csrc/, libtrimodal_hip.so) behind the C ABI of
include/trimodal_hip.h.  See DESIGN.md.
"""
from . import _lib  # noqa: F401  (does not load the .so until first use; load() raises loudly if it is missing)
from .modules import ConvDiscriminator, EmbeddingNet, PoseGenerator  # noqa: F401
from .optim import FusedAdam, ParamAdam  # noqa: F401
from .train_gan import GanTrainer, GraphedGanStep, StepLosses  # noqa: F401
from .vocab import Vocab  # noqa: F401
from .melspec import extract_melspectrogram  # noqa: F401
from .preprocess import DataPreprocessor, calculate_data_mean, resample_pose_seq  # noqa: F401
from .h36m import Human36M  # noqa: F401
from .rnn import GRU, EncoderRNN  # noqa: F401
from .seq2seq import Attn, BahdanauAttnDecoderRNN, Generator, Seq2SeqNet, train_iter_seq2seq  # noqa: F401
from .joint_embed import ContextEncoder, JointEmbedTrainer, PoseDecoderGRU, train_iter_embed  # noqa: F401
from .synthesize import generate_gestures, generate_gestures_batch  # noqa: F401
from . import checkpoint, config, data, ddp, eval_metrics, fgd, h36m, joint_embed, layers, melspec, ops, preprocess, resample, rnn, seq2seq, synthesize  # noqa: F401,E402  (hip.fgd, hip.config, ... as INTEGRATION.md uses them)

__all__ = ["PoseGenerator", "ConvDiscriminator", "EmbeddingNet", "FusedAdam", "ParamAdam", "GanTrainer", "GraphedGanStep", "StepLosses",
           "Vocab", "extract_melspectrogram", "DataPreprocessor", "calculate_data_mean", "resample_pose_seq", "Human36M", "GRU", "EncoderRNN",
           "Attn", "BahdanauAttnDecoderRNN", "Generator", "Seq2SeqNet", "train_iter_seq2seq", "ContextEncoder", "PoseDecoderGRU", "JointEmbedTrainer", "train_iter_embed", "generate_gestures",
           "generate_gestures_batch"]
