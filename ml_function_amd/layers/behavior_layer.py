"""AutoInt's interacting layer: the MI355X re-host of ProductAttentionLayer (behavior_layer.py:272-311) and
MultHeadAttentionLayer (:313-380) of the reference.  Reference quirks are kept on purpose: the "softmax" is a
sigmoid (:286,308), V is projected with key_w (:360; value_w exists but never receives a gradient), LayerNorm
epsilon is Keras' default 1e-3, the output is head-major [H,B,F,A].
Behaviour-sequence layers (extensions), each one fused kernel per direction with a composed torch path outside the kernel menu:
DinAttentionLayer (the Deep Interest Network's attention pooling), GRULayer (a GRU and the Deep Interest Evolution Network's AUGRU /
AGRU), TimeStreamGRULayer (the Deep Time-Stream model's GRU under an ODE over the event gaps), LSTMLayer / BiLSTMLayer (Keras' LSTM and Bidirectional(LSTM), the Deep Session Interest Network's session interest
interacting layer), SeqSelfAttentionLayer (the Behaviour Sequence Transformer's masked self-attention) and NTMMemoryLayer (the
Multi-channel user Interest Memory Network's Neural Turing Machine memory)."""
import torch

from .. import functional as Fn
from .base import Layer, _menu_fits


class ProductAttentionLayer(Layer):
    """Scaled product attention with a sigmoid in place of the softmax (behavior_layer.py:272-311).

    call([q, k, v], mask=None) -> sigmoid(q k^T [/ sqrt(A)] [masked]) v on the HIP path (fil_pattn_*: the scores never
    leave registers).  mask_mod 1 right-multiplies the scores by the float mask (:300-302), mask_mod 2 adds
    mask * (-100000) (:303-306).  Inside MultHeadAttentionLayer the same arithmetic runs fused with the projections,
    LayerNorm and residual (fil_attn_*) when there is no mask."""

    def __init__(self, use_scale=False, supports_masking=True, mask_mod=1):
        super().__init__()
        self.use_scale = use_scale
        self.supports_masking = supports_masking
        self.mask_mod = mask_mod

    def call(self, inputs, mask=None, **kwargs):
        q, k, v = inputs
        return Fn.product_attention(q, k, v, use_scale=self.use_scale, mask=mask, mask_mod=self.mask_mod)


class MultHeadAttentionLayer(Layer):
    """MultHeadAttentionLayer (behavior_layer.py:313-380).

    build creates query_w, key_w, value_w, res_w, each [K_in, head, dim] (glorot_uniform(seed); res_w uses Keras'
    default initializer, also glorot_uniform) and the LayerNormalization gamma/beta [dim].
    call(x [B,F,K], mask=None) -> [atten_v, res], both [H,B,F,A] (atten_v is [B,H,F,A] when head_concat; a single
    squeezed tensor when attention_head_dim == 1, like the reference :374-375)."""

    def __init__(self, attention_dim, attention_head_dim, seed=2020, use_scale=True, use_res=True, use_ln=True,
                 head_concat=False, supports_masking=True, atten_mask_mod=1, precision="f32"):
        super().__init__()
        self.precision = precision  # extension: "f16_mfma" = BASELINE config 5 (fp16 MFMA products, fp32 accumulate)
        self.attention_dim = attention_dim
        self.attention_head_dim = attention_head_dim
        self.attention_cal = ProductAttentionLayer(use_scale=use_scale, mask_mod=atten_mask_mod)
        self.seed = seed
        self.use_res = use_res
        self.use_ln = use_ln
        self.head_concat = head_concat
        self.supports_masking = supports_masking
        self.ln_epsilon = 1e-3  # tf.keras.layers.LayerNormalization() default

    def build(self, input_shape):
        shape = [input_shape[-1], self.attention_head_dim, self.attention_dim]
        self.query_w = self.add_weight("query_w", shape, "glorot_uniform", seed=self.seed)
        self.key_w = self.add_weight("key_w", shape, "glorot_uniform", seed=self.seed)
        self.value_w = self.add_weight("value_w", shape, "glorot_uniform", seed=self.seed)  # unused, as in the reference
        if self.use_res:
            self.res_w = self.add_weight("res_w", shape, "glorot_uniform")
        self.ln_gamma = self.add_weight("ln_gamma", [self.attention_dim], "ones")
        self.ln_beta = self.add_weight("ln_beta", [self.attention_dim], "zeros")
        super().build(input_shape)

    def _args(self):
        return (self.query_w, self.key_w, self.res_w if self.use_res else None,
                self.ln_gamma if self.use_ln else None, self.ln_beta if self.use_ln else None)

    def fits_fused_kernel(self, inputs):
        """The fused kernel's menu (include/fil.h): K <= 64, A <= 16, H <= 8, F <= 512, and the dynamic LDS footprint of BOTH the
        forward and the backward within the launchers' limit (163,328 bytes) in this layer's precision -- fil_attn_plan answers from
        the launchers' own arithmetic.  The backward's footprint is the larger one: in "f32" with 8 heads it ends the menu at F = 128
        (4 heads: F = 384), in "f16_mfma" with K = 64 at F = 208 (4 heads: F = 480).  A reference-legal layer outside the menu
        (e.g. attention_dim = 32, or 8 heads over 129 fields in f32) takes the composed path below instead of raising."""
        if inputs.dim() != 3:
            return False
        return _menu_fits(Fn.attn_plan, int(inputs.shape[1]), int(inputs.shape[2]), int(self.attention_head_dim), int(self.attention_dim),
                          self.precision)

    def _composed(self, inputs, mask):
        """The reference's op order (:358-369) with the attention core on the stand-alone kernel (fil_pattn_*: A <= 64, any mask) --
        projections as tensordot, ProductAttentionLayer([q, k, v], mask), LayerNormalization (epsilon 1e-3) by torch."""
        Wq, Wk, Wr, g, b = self._args()
        q = torch.tensordot(inputs, Wq, dims=1).permute(2, 0, 1, 3)
        k = torch.tensordot(inputs, Wk, dims=1).permute(2, 0, 1, 3)
        atten_v = self.attention_cal([q, k, k], mask=mask)                  # v is projected with key_w (:360)
        res = torch.tensordot(inputs, Wr, dims=1).permute(2, 0, 1, 3) if Wr is not None else None
        if g is not None:
            atten_v = torch.nn.functional.layer_norm(atten_v, (self.attention_dim,), g, b, self.ln_epsilon)
        return atten_v, res

    def fused_relu(self, inputs):
        """relu(res + LN(attention)) in one kernel: what DnnLayer(res_unit=1, other_dense=[self]) computes."""
        Wq, Wk, Wr, g, b = self._args()
        if not self.fits_fused_kernel(inputs):
            atten_v, res = self._composed(inputs, None)
            return torch.relu(atten_v + res) if res is not None else torch.relu(atten_v)
        return Fn.autoint_interact(inputs, Wq, Wk, Wr, g, b, use_scale=self.attention_cal.use_scale, eps=self.ln_epsilon,
                                   precision=self.precision)

    def call(self, inputs, mask=None, **kwargs):
        Wq, Wk, Wr, g, b = self._args()
        if mask is None and self.fits_fused_kernel(inputs):
            atten_v, res = Fn.mult_head_attention(inputs, Wq, Wk, Wr, g, b, use_scale=self.attention_cal.use_scale,
                                                  eps=self.ln_epsilon, precision=self.precision)
        else:
            # masked, or a shape outside the fused kernel's menu: the composed path
            atten_v, res = self._composed(inputs, mask)
        if res is None:
            res = []
        if self.head_concat:
            atten_v = atten_v.permute(1, 0, 2, 3)
        if self.attention_head_dim == 1:
            return atten_v.squeeze(0)
        return [atten_v, res]


def _check_seq_mask(who, mask, B, T):
    """The behaviour-sequence layers' mask: None, or a [B,T] bool / uint8 tensor (non-zero = live)."""
    if mask is not None and (tuple(mask.shape) != (B, T) or mask.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("%s: mask must be a [B,T] bool or uint8 tensor, got %s %s" % (who, tuple(mask.shape), mask.dtype))


def _masked_softmax(s, live):
    """The softmax of the scores s [B,T] over the live slots (live [B,T] bool; None = all live); a sample without a live slot gets
    weight 0 everywhere."""
    if live is not None:
        s = s.masked_fill(~live, float("-inf"))
    mx = s.max(dim=1, keepdim=True).values
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    w = torch.exp(s - mx)
    return w / w.sum(dim=1, keepdim=True).clamp_min(torch.finfo(w.dtype).tiny)      # no live slot: 0 / tiny = 0


_DIN_ACTIVATIONS = ("prelu", "relu", "sigmoid")


def din_attention_graph(q, keys, mask, w1, b1, alpha1, w2, b2, alpha2, w3, b3, softmax=False, activation="prelu"):
    """Fn.din_attention's math as torch ops on the tensors given (their dtype and device; autograd for the backward): the composed
    path of DinAttentionLayer and the comparator of its benchmark.  It materialises [B,T,4K] and [B,T,H1].  mask: [B,T] bool or None.
    A masked key is replaced by zero before anything reads it."""
    B, T, K = keys.shape
    live = torch.ones((B, T), dtype=torch.bool, device=keys.device) if mask is None else mask.to(torch.bool)
    keys = torch.where(live.unsqueeze(-1), keys, torch.zeros((), dtype=keys.dtype, device=keys.device))
    qe = q.unsqueeze(1).expand(B, T, K)
    x = torch.cat([qe, keys, qe - keys, qe * keys], dim=-1)
    if activation == "sigmoid":
        act = lambda u, a: torch.sigmoid(u)
    else:
        act = lambda u, a: torch.where(u > 0, u, a * u)
    h1 = act(torch.matmul(x, w1) + b1, alpha1)
    h2 = act(torch.matmul(h1, w2) + b2, alpha2)
    s = torch.matmul(h2, w3.reshape(-1, 1)).squeeze(-1) + b3.reshape(())
    a = _masked_softmax(s, live) if softmax else s * live.to(s.dtype)
    return (a.unsqueeze(-1) * keys).sum(dim=1)


class DinAttentionLayer(Layer):
    """The Deep Interest Network's attention pooling of a behaviour sequence (extension: the paper's activation unit; the
    reference's AttentionUnitLayer / ActivationUnitLayer are not restated here, their source was not available).

    call([query [B,1,K] or [B,K], keys [B,T,K]], mask=None) -> [B,1,K] = sum_t a_t k_t: the candidate scores every item of the
    history through Dense(H1) -> act -> Dense(H2) -> act -> Dense(1) on [q, k, q - k, q * k]; a_t is the score itself on the live
    slots (the paper; softmax=False) or the softmax of the scores over the live slots (softmax=True); scores are not scaled by
    sqrt(K).  mask: a [B,T] bool or uint8 tensor, non-zero = live (models.DINInput builds it as id != padding_id); None = all live.
    activation: "prelu" (Keras PReLU, a slope per unit, zeros-initialised), "relu" (the slopes frozen at 0) or "sigmoid" (no slopes).
    Dice is not offered (it needs batch statistics).  Weights: att_w1 [4K,H1], att_b1, att_alpha1, att_w2 [H1,H2], att_b2,
    att_alpha2, att_w3 [H2,1], att_b3 [1] -- glorot_uniform(seed), zeros, zeros: Keras' Dense and PReLU defaults.
    The MLP, the (masked) softmax and the weighted sum run in ONE HIP kernel per direction (Fn.din_attention, include/fil.h
    fil_din_*): no [B,T,4K] or [B,T,H1] tensor exists.  Outside the kernel menu (fits_kernel_menu) or for a non-fp32 input the
    layer takes the composed path -- the same graph in torch ops on the GPU, computed in fp32 -- instead of raising."""

    def __init__(self, hidden_units=(80, 40), activation="prelu", softmax=False, padding_id=0, seed=2020):
        super().__init__()
        hidden_units = tuple(int(h) for h in hidden_units)
        if len(hidden_units) != 2 or min(hidden_units) < 1:
            raise ValueError("DinAttentionLayer: hidden_units must be two positive widths, got %r" % (hidden_units,))
        if activation not in _DIN_ACTIVATIONS:
            raise ValueError("DinAttentionLayer: activation %r (%s)" % (activation, ", ".join(_DIN_ACTIVATIONS)))
        self.hidden_units = hidden_units
        self.activation = activation
        self.softmax = bool(softmax)
        self.padding_id = padding_id      # the id models.DINInput masks; the layer itself only sees the mask
        self.seed = seed

    def build(self, input_shape):
        k = int(input_shape[1][-1])
        h1, h2 = self.hidden_units
        self.att_w1 = self.add_weight("att_w1", [4 * k, h1], "glorot_uniform", seed=self.seed)
        self.att_b1 = self.add_weight("att_b1", [h1], "zeros")
        if self.activation != "sigmoid":
            self.att_alpha1 = self.add_weight("att_alpha1", [h1], "zeros", trainable=self.activation == "prelu")
        self.att_w2 = self.add_weight("att_w2", [h1, h2], "glorot_uniform", seed=self.seed)
        self.att_b2 = self.add_weight("att_b2", [h2], "zeros")
        if self.activation != "sigmoid":
            self.att_alpha2 = self.add_weight("att_alpha2", [h2], "zeros", trainable=self.activation == "prelu")
        self.att_w3 = self.add_weight("att_w3", [h2, 1], "glorot_uniform", seed=self.seed)
        self.att_b3 = self.add_weight("att_b3", [1], "zeros")
        super().build(input_shape)

    def _weights(self):
        sig = self.activation == "sigmoid"
        return (self.att_w1, self.att_b1, None if sig else self.att_alpha1, self.att_w2, self.att_b2, None if sig else self.att_alpha2,
                self.att_w3, self.att_b3)

    def fits_kernel_menu(self, query, keys):
        """fil_din_*'s menu (include/fil.h): K % 4 == 0, K <= 64, T <= 256, H1 <= 128, H2 <= 64, 4 K H1 + H1 H2 <= 16384 --
        fil_din_plan answers from the launchers' own arithmetic; the answer is cached per shape."""
        if keys.dim() != 3:
            return False
        return _menu_fits(Fn.din_plan, 1, int(keys.shape[1]), int(keys.shape[2]), *self.hidden_units)

    def _composed(self, q, keys, mask):
        """din_attention_graph on the GPU in fp32: a dozen launches and two [B,T,n] blocks per direction where the fused kernel makes
        none -- it exists so that a shape outside the kernel menu never raises."""
        Fn._require_cuda(q, keys, mask)      # (torch ops would run on a CPU tensor: there is no CPU path in this package)
        kernel_act = "sigmoid" if self.activation == "sigmoid" else "prelu"
        return din_attention_graph(q.to(torch.float32), keys.to(torch.float32), mask, *self._weights(), softmax=self.softmax,
                                   activation=kernel_act)

    def call(self, inputs, mask=None, **kwargs):
        query, keys = inputs
        if keys.dim() != 3 or query.dim() not in (2, 3) or query.numel() != keys.shape[0] * keys.shape[2]:
            raise ValueError("DinAttentionLayer: query must be [B,1,K] or [B,K] and keys [B,T,K], got %s and %s"
                             % (tuple(query.shape), tuple(keys.shape)))
        q = query.reshape(keys.shape[0], keys.shape[2])
        _check_seq_mask("DinAttentionLayer", mask, keys.shape[0], keys.shape[1])
        if q.dtype == torch.float32 and keys.dtype == torch.float32 and self.fits_kernel_menu(q, keys):
            pooled = Fn.din_attention(q, keys, mask, *self._weights(), softmax=self.softmax,
                                      activation="sigmoid" if self.activation == "sigmoid" else "prelu")
        else:
            pooled = self._composed(q, keys, mask)
        return pooled.unsqueeze(1)


_GRU_MODES = ("gru", "augru", "agru")


def gru_graph(x, a, mask, w, u, b, mode="gru", return_sequences=True):
    """Fn.gru's math as torch ops on the tensors given (their dtype and device; autograd for the backward), one step at a time: the
    composed path of GRULayer and the comparator of its benchmark -- about a dozen launches per step.  mask: [B,T] bool or None.
    x_t and a_t of a masked step are replaced by zero before anything reads them."""
    B, T, K = x.shape
    H = u.shape[0]
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    live = None if mask is None else mask.to(torch.bool)
    if live is not None:
        x = torch.where(live.unsqueeze(-1), x, zero)
        if a is not None:
            a = torch.where(live, a, zero)
    h = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    out = []
    for t in range(T):
        xp = torch.matmul(x[:, t], w) + b[0]
        hp = torch.matmul(h, u) + b[1]
        z = torch.sigmoid(xp[:, :H] + hp[:, :H])
        r = torch.sigmoid(xp[:, H:2 * H] + hp[:, H:2 * H])
        c = torch.tanh(xp[:, 2 * H:] + r * hp[:, 2 * H:])
        up = 1 - z
        if mode == "augru":
            up = a[:, t:t + 1] * up
        elif mode == "agru":
            up = a[:, t:t + 1].expand(B, H)
        hn = (1 - up) * h + up * c
        h = hn if live is None else torch.where(live[:, t:t + 1], hn, h)
        if return_sequences:
            out.append(h)
    return torch.stack(out, dim=1) if return_sequences else h


class GRULayer(Layer):
    """A GRU over a behaviour sequence, and the Deep Interest Evolution Network's attention-gated variants (extension: TF 2 Keras' GRU
    with its defaults -- reset_after=True, sigmoid / tanh, no dropout -- and the paper's AUGRU / AGRU, eq. 15-16).

    call(x [B,T,K], mask=None) with mode "gru"; call([x, scores [B,T]], mask=None) with "augru" (u' = a_t (1 - z)) or "agru"
    (u' = a_t) -> hs [B,T,units], or the last state [B,units] with return_sequences=False.  mask: a [B,T] bool or uint8 tensor,
    non-zero = live; a masked step repeats the state, zeros before the first live step (Keras' masking).  Weights carry Keras' names
    and defaults: kernel [K,3 units] glorot_uniform(seed), recurrent_kernel [units,3 units] orthogonal(seed), bias [2,3 units] zeros;
    the column order is z | r | h.  The whole recurrence runs in ONE HIP kernel per direction (Fn.gru, include/fil.h fil_gru_*).
    Outside the kernel menu (fits_kernel_menu) or for a non-fp32 input the layer takes the composed path -- gru_graph on the GPU,
    computed in fp32 -- instead of raising."""

    def __init__(self, units, mode="gru", return_sequences=True, seed=2020):
        super().__init__()
        if int(units) < 1:
            raise ValueError("GRULayer: units must be positive, got %r" % (units,))
        if mode not in _GRU_MODES:
            raise ValueError("GRULayer: mode %r (%s)" % (mode, ", ".join(_GRU_MODES)))
        self.units = int(units)
        self.mode = mode
        self.return_sequences = bool(return_sequences)
        self.seed = seed

    def build(self, input_shape):
        shape = input_shape[0] if isinstance(input_shape, list) else input_shape
        k, h = int(shape[-1]), self.units
        self.kernel = self.add_weight("kernel", [k, 3 * h], "glorot_uniform", seed=self.seed)
        self.recurrent_kernel = self.add_weight("recurrent_kernel", [h, 3 * h], "orthogonal", seed=self.seed)
        self.bias = self.add_weight("bias", [2, 3 * h], "zeros")
        super().build(input_shape)

    def fits_kernel_menu(self, x):
        """fil_gru_*'s menu (include/fil.h): K % 4 == 0, H % 4 == 0, K <= 64, H <= 64 -- fil_gru_plan answers from the launchers' own
        arithmetic; the answer is cached per shape."""
        if x.dim() != 3:
            return False
        return _menu_fits(Fn.gru_plan, 1, 1, int(x.shape[2]), self.units, self.mode)      # (the menu does not depend on T either)

    def _composed(self, x, scores, mask):
        """gru_graph on the GPU in fp32: about a dozen launches per step where the fused kernel makes one per direction -- it exists so
        that a shape outside the kernel menu never raises."""
        Fn._require_cuda(x, scores, mask)      # (torch ops would run on a CPU tensor: there is no CPU path in this package)
        return gru_graph(x.to(torch.float32), None if scores is None else scores.to(torch.float32), mask, self.kernel,
                         self.recurrent_kernel, self.bias, mode=self.mode, return_sequences=self.return_sequences)

    def call(self, inputs, mask=None, **kwargs):
        if self.mode == "gru":
            x, scores = (inputs[0] if isinstance(inputs, (list, tuple)) and len(inputs) == 1 else inputs), None
            if isinstance(x, (list, tuple)):
                raise ValueError("GRULayer: mode 'gru' takes x alone, got %d inputs" % len(x))
        else:
            if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
                raise ValueError("GRULayer: mode %r takes [x, scores]" % self.mode)
            x, scores = inputs
        if x.dim() != 3:
            raise ValueError("GRULayer: x must be [B,T,K], got %s" % (tuple(x.shape),))
        if scores is not None and tuple(scores.shape) != tuple(x.shape[:2]):
            raise ValueError("GRULayer: scores must be [B,T] = %s, got %s" % (tuple(x.shape[:2]), tuple(scores.shape)))
        _check_seq_mask("GRULayer", mask, x.shape[0], x.shape[1])
        if x.dtype == torch.float32 and (scores is None or scores.dtype == torch.float32) and self.fits_kernel_menu(x):
            return Fn.gru(x, scores, mask, self.kernel, self.recurrent_kernel, self.bias, mode=self.mode,
                          return_sequences=self.return_sequences)
        return self._composed(x, scores, mask)


class TimeStreamGRULayer(Layer):
    """A GRU over a behaviour sequence whose state moves through the time between the events (extension: the core of the Deep
    Time-Stream model; the reference's layer was not available).

    call([x [B,T,K], dt [B,T], dt_out [B] or None], mask=None): dt is the time from the previous live event to this one, dt_out the
    time from the last event to the prediction.  Before every live step the state follows dh/dt = tanh(h ode_kernel + ode_bias) for
    dt in `steps` explicit Euler substeps, then GRULayer's step (mode "gru") runs on it -> hs [B,T,units], or the last state
    [B,units] with return_sequences=False; with dt_out a pair (hs or last, z [B,units]), z = the last state moved on by dt_out.  mask
    as GRULayer's.  Weights: GRULayer's under its names and initialisers, ode_kernel [units,units] glorot_uniform(seed) and ode_bias
    [units] zeros.  The gaps are data and get no gradient.  The whole recurrence runs in ONE HIP kernel per direction (Fn.ts_gru,
    include/fil.h fil_tsgru_*).  Outside the kernel menu (fits_kernel_menu; more than 8 substeps are outside it) or for a non-fp32
    input the layer takes the composed path -- Fn.ts_gru_graph on the GPU, computed in fp32 -- instead of raising."""

    def __init__(self, units, steps=2, return_sequences=False, seed=2020):
        super().__init__()
        if int(units) < 1:
            raise ValueError("TimeStreamGRULayer: units must be positive, got %r" % (units,))
        if int(steps) != steps or int(steps) < 1:
            raise ValueError("TimeStreamGRULayer: steps must be a positive integer, got %r" % (steps,))
        self.units = int(units)
        self.steps = int(steps)
        self.return_sequences = bool(return_sequences)
        self.seed = seed

    def build(self, input_shape):
        shape = input_shape[0] if isinstance(input_shape, list) else input_shape
        k, h = int(shape[-1]), self.units
        self.kernel = self.add_weight("kernel", [k, 3 * h], "glorot_uniform", seed=self.seed)
        self.recurrent_kernel = self.add_weight("recurrent_kernel", [h, 3 * h], "orthogonal", seed=self.seed)
        self.bias = self.add_weight("bias", [2, 3 * h], "zeros")
        self.ode_kernel = self.add_weight("ode_kernel", [h, h], "glorot_uniform", seed=self.seed)
        self.ode_bias = self.add_weight("ode_bias", [h], "zeros")
        super().build(input_shape)

    def fits_kernel_menu(self, x):
        """fil_tsgru_*'s menu (include/fil.h): K % 4 == 0, H % 4 == 0, K <= 64, H <= 64, at most 8 substeps, and the LDS of both passes
        -- fil_tsgru_plan answers from the launchers' own arithmetic at the batch given (the tile, and with it the LDS, grows with
        every 4096 samples up to 64 samples a tile: the batch is rounded up to that step, so the cached answers stay few)."""
        if x.dim() != 3:
            return False
        batch = min(-(-max(int(x.shape[0]), 1) // 4096), 64) * 4096
        return _menu_fits(Fn.ts_gru_plan, batch, 1, int(x.shape[2]), self.units, self.steps)

    def _weights(self):
        return self.kernel, self.recurrent_kernel, self.bias, self.ode_kernel, self.ode_bias

    def _composed(self, x, dt, dt_out, mask):
        """Fn.ts_gru_graph on the GPU in fp32: about 10 + 4 steps launches per step where the fused kernel makes one per direction --
        it exists so that a shape outside the kernel menu never raises."""
        Fn._require_cuda(x, dt, dt_out, mask)      # (torch ops would run on a CPU tensor: there is no CPU path in this package)
        f32 = lambda t: None if t is None else t.to(torch.float32)
        return Fn.ts_gru_graph(f32(x), f32(dt), f32(dt_out), mask, *self._weights(), steps=self.steps,
                               return_sequences=self.return_sequences)

    def call(self, inputs, mask=None, **kwargs):
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 3:
            raise ValueError("TimeStreamGRULayer: the call takes [x, dt, dt_out or None]")
        x, dt, dt_out = inputs
        if x.dim() != 3:
            raise ValueError("TimeStreamGRULayer: x must be [B,T,K], got %s" % (tuple(x.shape),))
        if dt is None or tuple(dt.shape) != tuple(x.shape[:2]) or (dt_out is not None and tuple(dt_out.shape) != (x.shape[0],)):
            raise ValueError("TimeStreamGRULayer: dt must be [B,T] = %s and dt_out [B] or None, got %s and %s"
                             % (tuple(x.shape[:2]), None if dt is None else tuple(dt.shape), None if dt_out is None else tuple(dt_out.shape)))
        if dt.requires_grad or (dt_out is not None and dt_out.requires_grad):
            raise ValueError("TimeStreamGRULayer: dt / dt_out requires grad -- the gaps are data, there is no gradient to them")
        _check_seq_mask("TimeStreamGRULayer", mask, x.shape[0], x.shape[1])
        if all(t is None or t.dtype == torch.float32 for t in (x, dt, dt_out)) and self.fits_kernel_menu(x):
            return Fn.ts_gru(x, dt, dt_out, mask, *self._weights(), steps=self.steps, return_sequences=self.return_sequences)
        return self._composed(x, dt, dt_out, mask)


_LSTM_DIRECTIONS = ("forward", "reverse", "bidirectional")


def lstm_graph(x, mask, w, u, b, direction="forward", return_sequences=True):
    """Fn.lstm's math as torch ops on the tensors given (their dtype and device; autograd for the backward), one step at a time: the
    composed path of LSTMLayer / BiLSTMLayer and the comparator of their benchmark -- about a dozen launches per step and direction.
    mask: [B,T] bool or None.  x_t of a masked step is replaced by zero before anything reads it.  "bidirectional": w [2,K,4H],
    u [2,H,4H], b [2,4H] -> [B,T,2H] (or the two last states [B,2H]), the forward direction first."""
    if direction == "bidirectional":
        return torch.cat([lstm_graph(x, mask, w[i], u[i], b[i], d, return_sequences) for i, d in enumerate(_LSTM_DIRECTIONS[:2])], dim=-1)
    B, T, K = x.shape
    H = u.shape[0]
    live = None if mask is None else mask.to(torch.bool)
    if live is not None:
        x = torch.where(live.unsqueeze(-1), x, torch.zeros((), dtype=x.dtype, device=x.device))
    h = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    c = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    out = [None] * T
    for t in (range(T - 1, -1, -1) if direction == "reverse" else range(T)):
        z = torch.matmul(x[:, t], w) + torch.matmul(h, u) + b
        i, f, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.sigmoid(z[:, 3 * H:])
        cn = f * c + i * torch.tanh(z[:, 2 * H:3 * H])
        hn = o * torch.tanh(cn)
        if live is not None:
            cn, hn = torch.where(live[:, t:t + 1], cn, c), torch.where(live[:, t:t + 1], hn, h)
        h, c = hn, cn
        out[t] = h
    return torch.stack(out, dim=1) if return_sequences else h


class _LstmBase(Layer):
    """What LSTMLayer and BiLSTMLayer share: the input checks and the choice between the fused op and the composed path."""

    direction = None

    def _weights(self):
        raise NotImplementedError

    def fits_kernel_menu(self, x):
        """fil_lstm_*'s menu (include/fil.h): K % 4 == 0, H % 4 == 0, K <= 64, H <= 64 and both passes within the LDS limit (every such
        shape with H <= 56, H = 60 with K <= 52, H = 64 with K <= 40) -- fil_lstm_plan answers from the launchers' own arithmetic;
        the answer is cached per shape."""
        if x.dim() != 3:
            return False
        return _menu_fits(Fn.lstm_plan, 1, 1, int(x.shape[2]), self.units, self.direction)      # (the menu does not depend on T)

    def _composed(self, x, mask):
        """lstm_graph on the GPU in fp32: about a dozen launches per step and direction where the fused kernel makes one per pass --
        it exists so that a shape outside the kernel menu never raises."""
        Fn._require_cuda(x, mask)      # (torch ops would run on a CPU tensor: there is no CPU path in this package)
        return lstm_graph(x.to(torch.float32), mask, *self._weights(), direction=self.direction, return_sequences=self.return_sequences)

    def _run(self, x, mask):
        who = type(self).__name__
        if not torch.is_tensor(x) or x.dim() != 3:
            raise ValueError("%s: x must be [B,T,K], got %s" % (who, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        _check_seq_mask(who, mask, x.shape[0], x.shape[1])
        if x.dtype == torch.float32 and self.fits_kernel_menu(x):
            return Fn.lstm(x, mask, *self._weights(), direction=self.direction, return_sequences=self.return_sequences)
        return self._composed(x, mask)


def _lstm_bias(p):
    """Keras' LSTM bias with unit_forget_bias=True: zeros, the forget block (the second quarter) at ones."""
    with torch.no_grad():
        p.zero_()
        h = p.shape[0] // 4
        p[h:2 * h] = 1.0


class LSTMLayer(_LstmBase):
    """An LSTM over a sequence (extension: TF 2 Keras' LSTM with its defaults -- sigmoid / tanh, unit_forget_bias, no dropout).

    call(x [B,T,K], mask=None) -> hs [B,T,units], or the last state [B,units] with return_sequences=False.  go_backwards=True walks
    t = T-1 .. 0; the sequence it returns is turned back, so hs[:, t] is the state reached after step t and the last state is
    hs[:, 0] (Keras returns the walking order: flip(1) gives it).  mask: a [B,T] bool or uint8 tensor, non-zero = live; a masked step
    repeats both states, zeros before the first live step (Keras' masking).  Weights carry Keras' names and defaults: kernel
    [K,4 units] glorot_uniform(seed), recurrent_kernel [units,4 units] orthogonal(seed), bias [4 units] zeros with the forget block at
    ones; the column order is i | f | c | o.  The whole recurrence runs in ONE HIP kernel per pass (Fn.lstm, include/fil.h
    fil_lstm_*).  Outside the kernel menu (fits_kernel_menu) or for a non-fp32 input the layer takes the composed path -- lstm_graph
    on the GPU, computed in fp32 -- instead of raising."""

    def __init__(self, units, return_sequences=True, go_backwards=False, seed=2020):
        super().__init__()
        if int(units) < 1:
            raise ValueError("LSTMLayer: units must be positive, got %r" % (units,))
        self.units = int(units)
        self.return_sequences = bool(return_sequences)
        self.go_backwards = bool(go_backwards)
        self.direction = "reverse" if self.go_backwards else "forward"
        self.seed = seed

    def build(self, input_shape):
        k, h = int(input_shape[-1]), self.units
        self.kernel = self.add_weight("kernel", [k, 4 * h], "glorot_uniform", seed=self.seed)
        self.recurrent_kernel = self.add_weight("recurrent_kernel", [h, 4 * h], "orthogonal", seed=self.seed)
        self.bias = self.add_weight("bias", [4 * h], _lstm_bias)
        super().build(input_shape)

    def _weights(self):
        return self.kernel, self.recurrent_kernel, self.bias

    def call(self, inputs, mask=None, **kwargs):
        return self._run(inputs, mask)


_MERGE_MODES = ("concat", "sum", "ave")


class BiLSTMLayer(_LstmBase):
    """Keras' Bidirectional(LSTM(units)) (extension; the session interest interacting layer of the Deep Session Interest Network).

    call(x [B,T,K], mask=None) -> [B,T,2 units] with merge_mode "concat" (the forward direction first), [B,T,units] with "sum" or
    "ave"; with return_sequences=False the directions' last states (the forward one's after t = T-1, the backward one's after t = 0)
    merged the same way.  Weights: forward_kernel, forward_recurrent_kernel, forward_bias and backward_* with LSTMLayer's shapes and
    initialisers (the backward direction seeded with seed + 1).  Both directions run in ONE launch per pass (Fn.lstm with direction
    "bidirectional"), which writes the concatenation; "sum" and "ave" are torch ops on its two halves.  Masking, the kernel menu and
    the composed path are LSTMLayer's."""

    direction = "bidirectional"

    def __init__(self, units, merge_mode="concat", return_sequences=True, seed=2020):
        super().__init__()
        if int(units) < 1:
            raise ValueError("BiLSTMLayer: units must be positive, got %r" % (units,))
        if merge_mode not in _MERGE_MODES:
            raise ValueError("BiLSTMLayer: merge_mode %r (%s)" % (merge_mode, ", ".join(_MERGE_MODES)))
        self.units = int(units)
        self.merge_mode = merge_mode
        self.return_sequences = bool(return_sequences)
        self.seed = seed

    def build(self, input_shape):
        k, h = int(input_shape[-1]), self.units
        for n, name in enumerate(("forward", "backward")):
            setattr(self, name + "_kernel", self.add_weight(name + "_kernel", [k, 4 * h], "glorot_uniform", seed=self.seed + n))
            setattr(self, name + "_recurrent_kernel", self.add_weight(name + "_recurrent_kernel", [h, 4 * h], "orthogonal", seed=self.seed + n))
            setattr(self, name + "_bias", self.add_weight(name + "_bias", [4 * h], _lstm_bias))
        super().build(input_shape)

    def _weights(self):
        return (torch.stack([self.forward_kernel, self.backward_kernel]),
                torch.stack([self.forward_recurrent_kernel, self.backward_recurrent_kernel]),
                torch.stack([self.forward_bias, self.backward_bias]))

    def call(self, inputs, mask=None, **kwargs):
        out = self._run(inputs, mask)
        if self.merge_mode == "concat":
            return out
        fwd, bwd = out[..., :self.units], out[..., self.units:]
        return fwd + bwd if self.merge_mode == "sum" else (fwd + bwd) * 0.5


NTM_EPS = 1e-6


def ntm_cosine(M, k):
    """The memory's content addressing: c_i = (M_i . k) / sqrt((|M_i|^2 + eps)(|k|^2 + eps)) for M [B,m,D] and k [B,D] -> [B,m]; one
    square root of the product, smooth at M_i = 0 and at k = 0."""
    dot = (M * k.unsqueeze(1)).sum(-1)
    return dot / torch.sqrt(((M * M).sum(-1) + NTM_EPS) * ((k * k).sum(-1, keepdim=True) + NTM_EPS))


def ntm_beta(p):
    """The sharpness of an addressing softmax: softplus(p) + 1, softplus(v) = max(v, 0) + log1p(exp(-|v|))."""
    return torch.clamp_min(p, 0) + torch.log1p(torch.exp(-torch.abs(p))) + 1


def ntm_address(M, k, beta):
    """softmax_i(beta c_i(k)) for M [B,m,D], k [B,D], beta [B,1] or a scalar -> [B,m], the row maximum subtracted."""
    s = beta * ntm_cosine(M, k)
    w = torch.exp(s - s.max(dim=1, keepdim=True).values)
    return w / w.sum(dim=1, keepdim=True)


def ntm_memory_graph(h, mask, wp, bp, m0, return_sequences=True):
    """Fn.ntm_memory's math as torch ops on the tensors given (their dtype and device; autograd for the backward), one step at a time:
    the composed path of NTMMemoryLayer and the comparator of its benchmark -- about thirty launches per step.  mask: [B,T] bool or
    None.  h_t of a masked step is replaced by zero before anything reads it.  -> (rs [B,T,D] or the last read [B,D], M_T [B,m,D])."""
    B, T, H = h.shape
    m, D = m0.shape
    live = None if mask is None else mask.to(torch.bool)
    if live is not None:
        h = torch.where(live.unsqueeze(-1), h, torch.zeros((), dtype=h.dtype, device=h.device))
    M = m0.unsqueeze(0).expand(B, m, D)
    r = torch.zeros((B, D), dtype=h.dtype, device=h.device)
    out = []
    for t in range(T):
        p = torch.matmul(h[:, t], wp) + bp
        kr, kw = torch.tanh(p[:, :D]), torch.tanh(p[:, D:2 * D])
        e, a = torch.sigmoid(p[:, 2 * D:3 * D]), torch.tanh(p[:, 3 * D:4 * D])
        wr = ntm_address(M, kr, ntm_beta(p[:, 4 * D:4 * D + 1]))
        ww = ntm_address(M, kw, ntm_beta(p[:, 4 * D + 1:4 * D + 2])).unsqueeze(-1)
        rn = (wr.unsqueeze(-1) * M).sum(1)
        Mn = M * (1 - ww * e.unsqueeze(1)) + ww * a.unsqueeze(1)
        if live is not None:
            lt = live[:, t:t + 1]
            rn, Mn = torch.where(lt, rn, r), torch.where(lt.unsqueeze(-1), Mn, M)
        r, M = rn, Mn
        if return_sequences:
            out.append(r)
    return (torch.stack(out, dim=1) if return_sequences else r), M.contiguous()


def _ntm_initial_memory(seed):
    """The initial memory's initialiser: normal with std 0.1 from the seed -- the rows must differ, or the slots never separate."""
    def init(p):
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
        with torch.no_grad():
            p.copy_((torch.randn(tuple(p.shape), generator=gen, dtype=torch.float32) * 0.1).to(p.device))
    return init


class NTMMemoryLayer(Layer):
    """A Neural Turing Machine memory over a sequence (extension: the memory of the Multi-channel user Interest Memory Network, the
    paper's section 4.1; the reference's ReadLayer / WriteLayer / AddressCalLayer / ControlWrapLayer are not restated, their source
    was not available).

    call(h [B,T,H], mask=None) -> [last read [B,D], final memory [B,m,D]], the reads [B,T,D] first with return_sequences=True;
    m = memory_slots, D = memory_dim (None: the input width H).  h are the controller's states (in models.MIMN a GRULayer's output):
    the controller sees the history only, the read is not fed back.  Per live step one Dense(4D + 2) of h_t gives the read key, the
    write key, the erase and add vectors and the two sharpnesses; both heads address the slots by cosine similarity on the previous
    memory; the read comes before the erase-then-add write.  mask: a [B,T] bool or uint8 tensor, non-zero = live; a masked step
    carries the memory and the read (zeros before the first live step).  Weights: read_write_kernel [H,4D+2] glorot_uniform(seed),
    read_write_bias [4D+2] zeros, initial_memory [m,D] normal(std 0.1) from the seed, shared by all samples.  The whole recurrence
    runs in ONE HIP kernel per direction (Fn.ntm_memory, include/fil.h fil_ntm_*).  Outside the kernel menu (fits_kernel_menu) or for
    a non-fp32 input the layer takes the composed path -- ntm_memory_graph on the GPU, computed in fp32 -- instead of raising."""

    def __init__(self, memory_slots=4, memory_dim=None, return_sequences=False, seed=2020):
        super().__init__()
        if int(memory_slots) < 1:
            raise ValueError("NTMMemoryLayer: memory_slots must be positive, got %r" % (memory_slots,))
        if memory_dim is not None and int(memory_dim) < 1:
            raise ValueError("NTMMemoryLayer: memory_dim must be positive or None, got %r" % (memory_dim,))
        self.memory_slots = int(memory_slots)
        self.memory_dim = None if memory_dim is None else int(memory_dim)
        self.return_sequences = bool(return_sequences)
        self.seed = seed

    def build(self, input_shape):
        h = int(input_shape[-1])
        d = self.memory_dim or h
        self.read_write_kernel = self.add_weight("read_write_kernel", [h, 4 * d + 2], "glorot_uniform", seed=self.seed)
        self.read_write_bias = self.add_weight("read_write_bias", [4 * d + 2], "zeros")
        self.initial_memory = self.add_weight("initial_memory", [self.memory_slots, d], _ntm_initial_memory(self.seed))
        super().build(input_shape)

    def _weights(self):
        return self.read_write_kernel, self.read_write_bias, self.initial_memory

    def fits_kernel_menu(self, h):
        """fil_ntm_*'s menu (include/fil.h): H % 4 == 0, D % 4 == 0, H <= 64, D <= 64, m <= 16 -- fil_ntm_plan answers from the
        launchers' own arithmetic; the answer is cached per shape."""
        if h.dim() != 3:
            return False
        return _menu_fits(Fn.ntm_plan, 1, 1, int(h.shape[2]), self.memory_slots, int(self.initial_memory.shape[1]))      # (the menu does not depend on T)

    def _composed(self, h, mask):
        """ntm_memory_graph on the GPU in fp32: about thirty launches per step where the fused kernel makes one per direction -- it
        exists so that a shape outside the kernel menu never raises."""
        Fn._require_cuda(h, mask)      # (torch ops would run on a CPU tensor: there is no CPU path in this package)
        return ntm_memory_graph(h.to(torch.float32), mask, *self._weights(), return_sequences=self.return_sequences)

    def call(self, inputs, mask=None, **kwargs):
        h = inputs[0] if isinstance(inputs, (list, tuple)) and len(inputs) == 1 else inputs
        if not torch.is_tensor(h) or h.dim() != 3:
            raise ValueError("NTMMemoryLayer: h must be [B,T,H], got %s" % (tuple(h.shape) if torch.is_tensor(h) else type(h).__name__,))
        if h.shape[2] != self.read_write_kernel.shape[0]:
            raise ValueError("NTMMemoryLayer: built for H = %d, got %s" % (self.read_write_kernel.shape[0], tuple(h.shape)))
        _check_seq_mask("NTMMemoryLayer", mask, h.shape[0], h.shape[1])
        if h.dtype == torch.float32 and self.fits_kernel_menu(h):
            out, mem = Fn.ntm_memory(h, mask, *self._weights(), return_sequences=self.return_sequences)
        else:
            out, mem = self._composed(h, mask)
        return [out, mem]


def seq_self_attention_graph(x, mask, wq, wk, wv, heads, use_scale=True):
    """Fn.seq_self_attention's math as torch ops on the tensors given (their dtype and device; autograd for the backward): the
    composed path of SeqSelfAttentionLayer and the comparator of its benchmark -- three small GEMMs, a [B,H,T,T] score block written
    and read several times, about a dozen launches per direction.  mask: [B,T] bool / uint8 or None.  The x row of a masked position
    is replaced by zero before anything reads it; a masked key gets weight 0, a masked row (and a sample with no live slot) is 0."""
    B, T, K = x.shape
    H = int(heads)
    D = wq.shape[1] // H
    live = None if mask is None else mask.to(torch.bool)
    if live is not None:
        x = torch.where(live.unsqueeze(-1), x, torch.zeros((), dtype=x.dtype, device=x.device))
    q = torch.matmul(x, wq).reshape(B, T, H, D).permute(0, 2, 1, 3)
    k = torch.matmul(x, wk).reshape(B, T, H, D).permute(0, 2, 1, 3)
    v = torch.matmul(x, wv).reshape(B, T, H, D).permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2))
    if use_scale:
        s = s * (1.0 / float(D) ** 0.5)
    if live is not None:
        key_live = live.reshape(B, 1, 1, T)
        s = torch.where(key_live, s, torch.full((), -float("inf"), dtype=s.dtype, device=s.device))
        m = torch.where(live.any(dim=1).reshape(B, 1, 1, 1), s.detach().max(dim=-1, keepdim=True).values,
                        torch.zeros((), dtype=s.dtype, device=s.device))
        e = torch.where(key_live, torch.exp(s - m), torch.zeros((), dtype=s.dtype, device=s.device))
        p = e / e.sum(dim=-1, keepdim=True).clamp_min(torch.finfo(s.dtype).tiny)
    else:
        p = torch.softmax(s, dim=-1)
    out = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, T, H * D)
    if live is not None:
        out = torch.where(live.unsqueeze(-1), out, torch.zeros((), dtype=out.dtype, device=out.device))
    return out


class SeqSelfAttentionLayer(Layer):
    """Masked multi-head scaled dot-product self-attention over a behaviour sequence (extension: the layer of "Attention is all you
    need" as the Behaviour Sequence Transformer applies it to a history; MultHeadAttentionLayer above keeps the reference's quirks and
    is a different layer).

    call(x [B,T,K], mask=None) -> [B,T,heads * head_dim], heads concatenated.  mask: a [B,T] bool or uint8 tensor, non-zero = live;
    the softmax runs over the live keys and a masked position's row is 0.  Weights carry the reference layer's names and shape:
    query_w, key_w, value_w, each [K, heads, head_dim], glorot_uniform(seed) -- and value_w is used here.  No biases, no output
    projection, no dropout (SeqViewAttentionLayer adds the causal and the cross mask).  One HIP kernel per direction
    (Fn.seq_self_attention, include/fil.h fil_seqattn_*).
    Outside the kernel menu (fits_kernel_menu) or for a non-fp32 input the layer takes the composed path -- seq_self_attention_graph
    on the GPU, computed in fp32 -- instead of raising."""

    def __init__(self, heads, head_dim, use_scale=True, seed=2020):
        super().__init__()
        if int(heads) < 1 or int(head_dim) < 1:
            raise ValueError("SeqSelfAttentionLayer: heads and head_dim must be positive, got %r and %r" % (heads, head_dim))
        self.heads = int(heads)
        self.head_dim = int(head_dim)
        self.use_scale = bool(use_scale)
        self.seed = seed

    def build(self, input_shape):
        k = int(input_shape[-1])
        shape = [k, self.heads, self.head_dim]
        self.query_w = self.add_weight("query_w", shape, "glorot_uniform", seed=self.seed)
        self.key_w = self.add_weight("key_w", shape, "glorot_uniform", seed=self.seed)
        self.value_w = self.add_weight("value_w", shape, "glorot_uniform", seed=self.seed)
        super().build(input_shape)

    def fits_kernel_menu(self, x):
        """fil_seqattn_*'s menu (include/fil.h): K % 4 == 0, D % 4 == 0, K <= 64, H <= 8, H D <= 64, T <= 256 and a one-sample tile
        within the LDS limit -- fil_seqattn_plan answers from the launchers' own arithmetic; the answer is cached per shape."""
        if x.dim() != 3:
            return False
        return x.shape[1] >= 1 and _menu_fits(Fn.seq_attn_plan, 1, int(x.shape[1]), int(x.shape[2]), self.heads, self.head_dim)

    def _flat(self):
        hd = self.heads * self.head_dim
        return tuple(w.reshape(w.shape[0], hd) for w in (self.query_w, self.key_w, self.value_w))

    def _composed(self, x, mask):
        """seq_self_attention_graph on the GPU in fp32: it exists so that a shape outside the kernel menu never raises."""
        Fn._require_cuda(x, mask)      # (torch ops would run on a CPU tensor: there is no CPU path in this package)
        return seq_self_attention_graph(x.to(torch.float32), mask, *self._flat(), self.heads, use_scale=self.use_scale)

    def call(self, inputs, mask=None, **kwargs):
        x = inputs
        if not torch.is_tensor(x) or x.dim() != 3:
            raise ValueError("SeqSelfAttentionLayer: x must be [B,T,K], got %s" % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
        _check_seq_mask("SeqSelfAttentionLayer", mask, x.shape[0], x.shape[1])
        if x.dtype == torch.float32 and self.fits_kernel_menu(x):
            return Fn.seq_self_attention(x, mask, *self._flat(), self.heads, use_scale=self.use_scale)
        return self._composed(x, mask)


def seq_view_attention_graph(x, mask, wq, wk, wv, heads, use_scale=True, view="full", split=0, pool=False):
    """Fn.seq_view_attention's math as torch ops on the tensors given (their dtype and device; autograd for the backward): the
    composed path of SeqViewAttentionLayer and the comparator of its benchmark.  On top of seq_self_attention_graph's launches it
    builds the view's [T,T] structure mask and broadcasts it over the [B,H,T,T] score block, and the pooled form adds a masked mean
    over the rows.  A row that may see no live key is 0 and sends no gradient; a sample without a live row pools to 0."""
    Fn.seq_view_check("seq_view_attention_graph", view, split, x.shape[1])
    B, T, K = x.shape
    H = int(heads)
    D = wq.shape[1] // H
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    live = torch.ones((B, T), dtype=torch.bool, device=x.device) if mask is None else mask.to(torch.bool)
    if mask is not None:
        x = torch.where(live.unsqueeze(-1), x, zero)
    q = torch.matmul(x, wq).reshape(B, T, H, D).permute(0, 2, 1, 3)
    k = torch.matmul(x, wk).reshape(B, T, H, D).permute(0, 2, 1, 3)
    v = torch.matmul(x, wv).reshape(B, T, H, D).permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2))
    if use_scale:
        s = s * (1.0 / float(D) ** 0.5)
    allowed = live.reshape(B, 1, 1, T)
    if view != "full":
        pos = torch.arange(T, device=x.device)
        if view == "causal":
            structure = pos.reshape(1, T) <= pos.reshape(T, 1)
        else:
            structure = (pos.reshape(T, 1) < int(split)) != (pos.reshape(1, T) < int(split))
        allowed = allowed & structure.reshape(1, 1, T, T)
    s = torch.where(allowed, s, torch.full((), -float("inf"), dtype=s.dtype, device=s.device))
    some = allowed.any(dim=-1, keepdim=True)
    m = torch.where(some, s.detach().max(dim=-1, keepdim=True).values, zero)
    e = torch.where(allowed, torch.exp(s - m), zero)
    p = e / e.sum(dim=-1, keepdim=True).clamp_min(torch.finfo(s.dtype).tiny)
    out = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, T, H * D)
    out = torch.where(live.unsqueeze(-1), out, zero)
    if not pool:
        return out
    n = live.sum(dim=1, keepdim=True).to(out.dtype)
    return torch.where(n > 0, out.sum(dim=1) / n.clamp_min(1.0), zero)


class SeqViewAttentionLayer(SeqSelfAttentionLayer):
    """SeqSelfAttentionLayer under a structure mask, with an optional mean over the rows (extension: a view of the Sequence-Aware
    Factorization Machine and its intra-view pooling).

    view: "full"; "causal" -- row i sees the live keys j <= i; "cross" -- the first `split` rows (the static block) see only the live
    keys of the others (the history) and the others only theirs, 1 <= split <= T-1.  A live row with no key to see is 0.  pool=True:
    call(x [B,T,K], mask=None) -> [B, heads * head_dim], the mean of the live rows, taken inside the kernel (Fn.seq_view_attention:
    no [B,T,H D] tensor in either direction).  The weights, their names, the kernel menu and the composed path outside it (here
    seq_view_attention_graph) are SeqSelfAttentionLayer's."""

    def __init__(self, heads, head_dim, use_scale=True, seed=2020, view="full", split=0, pool=False):
        super().__init__(heads, head_dim, use_scale=use_scale, seed=seed)
        Fn.seq_view_check("SeqViewAttentionLayer", view, split)
        self.view = view
        self.split = int(split)
        self.pool = bool(pool)

    def _composed(self, x, mask):
        """seq_view_attention_graph on the GPU in fp32: it exists so that a shape outside the kernel menu never raises."""
        Fn._require_cuda(x, mask)
        return seq_view_attention_graph(x.to(torch.float32), mask, *self._flat(), self.heads, use_scale=self.use_scale, view=self.view,
                                        split=self.split, pool=self.pool)

    def call(self, inputs, mask=None, **kwargs):
        x = inputs
        if not torch.is_tensor(x) or x.dim() != 3:
            raise ValueError("SeqViewAttentionLayer: x must be [B,T,K], got %s" % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
        _check_seq_mask("SeqViewAttentionLayer", mask, x.shape[0], x.shape[1])
        Fn.seq_view_check("SeqViewAttentionLayer", self.view, self.split, x.shape[1])
        if x.dtype == torch.float32 and self.fits_kernel_menu(x):
            return Fn.seq_view_attention(x, mask, *self._flat(), self.heads, use_scale=self.use_scale, view=self.view, split=self.split,
                                         pool=self.pool)
        return self._composed(x, mask)
