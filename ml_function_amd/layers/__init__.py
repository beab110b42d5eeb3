from ..capture import capture_step
from .base import Layer
from .behavior_layer import (BiLSTMLayer, DinAttentionLayer, GRULayer, LSTMLayer, MultHeadAttentionLayer, NTMMemoryLayer, ProductAttentionLayer,
                             SeqSelfAttentionLayer, SeqViewAttentionLayer, TimeStreamGRULayer)
from .core_layer import (AlignLayer, Dense, DnnLayer, HiddenLayer, IntraViewPoolingLayer, MergeScoreLayer, ResActivateLayer, ScoreLayer,
                         StackLayer)
from .interactive_layer import (CIN, AFMLayer, AttentionBaseLayer, BagEmbed, CrossLayer, ExtractLayer, FmLayer, InnerLayer, IPnnLayer, LinearLayer,
                                OPnnLayer, SparseEmbed)

__all__ = ["capture_step", "Layer", "InnerLayer", "FmLayer", "CrossLayer", "CIN", "SparseEmbed", "ProductAttentionLayer",
           "MultHeadAttentionLayer", "StackLayer", "ScoreLayer", "MergeScoreLayer", "HiddenLayer", "ResActivateLayer",
           "DnnLayer", "Dense", "IPnnLayer", "OPnnLayer", "LinearLayer", "AttentionBaseLayer", "ExtractLayer",
           "IntraViewPoolingLayer", "AlignLayer", "BagEmbed", "AFMLayer", "DinAttentionLayer", "GRULayer",
           "SeqSelfAttentionLayer", "LSTMLayer", "BiLSTMLayer", "SeqViewAttentionLayer", "NTMMemoryLayer", "TimeStreamGRULayer"]
