"""LstmLastHiddenModule and LstmConcatAverageModule (reference: rnn_modules.py:20-53, :56-88): a stack of TF1
``BasicLSTMCell(lstm_size, forget_bias=1.0)`` under ``tf.nn.dynamic_rnn(sequence_length=...)``.

Variables carry TF's names: ``rnn/multi_rnn_cell/cell_<l>/basic_lstm_cell/kernel`` [In_l + H, 4H] (glorot-uniform, TF's default for an
uninitialised ``get_variable``) and ``.../bias`` [4H] (zeros); the kernel's columns are gate-major ``i | j | f | o``.  Layer l > 0 reads
layer l - 1's zero-padded outputs.

On the GPU with FLAGS.lstm_fused and a hidden size ops.lstm_layer_ok accepts (a multiple of 128) every layer is ONE ops.lstm_layer call:
a kernel per time step each way on exact-fp32 MFMAs (csrc/lstm.hip), the non-recurrent products as large GEMMs around the loop.
Otherwise -- the flag off, another hidden size, the CPU -- ``_lstm_layer_host`` runs the same layer as a per-step torch formulation.  The
variables and the results are the same either way.
"""
from __future__ import annotations

import torch

from . import FLAGS, layers, modules, ops
from . import variables as vs

FORGET_BIAS = 1.0


def _lstm_layer_host(x, kernel, bias, lengths, forget_bias=FORGET_BIAS):
    """x [B, T, In], kernel [In + H, 4H], bias [4H], lengths [B] -> (outputs [B, T, H], h_last [B, H], c_last [B, H]) in torch, one
    step at a time: z = [x_t, h] kernel + bias = i | j | f | o; c' = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j); h' = tanh(c')
    sigmoid(o).  From t = min(lengths[b], T) on the state is copied through and the output row is zero."""
    B, T, In = x.shape
    H = bias.shape[0] // 4
    xw = (x.reshape(B * T, In).matmul(kernel[:In]) + bias).reshape(B, T, 4 * H)
    wh = kernel[In:]
    h = c = x.new_zeros(B, H)
    zero = x.new_zeros(B, H)
    valid = torch.arange(T, device=x.device).unsqueeze(0) < lengths.to(x.device).reshape(B, 1)
    outputs = []
    for t in range(T):
        i, j, f, o = (xw[:, t] + h.matmul(wh)).split(H, dim=1)
        c_new = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
        h_new = torch.tanh(c_new) * torch.sigmoid(o)
        m = valid[:, t:t + 1]
        c, h = torch.where(m, c_new, c), torch.where(m, h_new, h)
        outputs.append(torch.where(m, h_new, zero))
    return torch.stack(outputs, 1), h, c


def lstm_layer(x, kernel, bias, lengths, forget_bias=FORGET_BIAS):
    """One layer on the route the flags and the shapes select (see the module docstring)."""
    if FLAGS.lstm_fused and x.is_cuda and x.dtype == torch.float32 and ops.lstm_layer_ok(x.shape[0], x.shape[1], bias.shape[0] // 4):
        return ops.lstm_layer(x, kernel, bias, lengths, forget_bias)
    return _lstm_layer_host(x, kernel, bias, lengths, forget_bias)


def _stacked_lstm(inputs, lengths, lstm_size, num_layers):
    """MultiRNNCell of num_layers BasicLSTMCells under dynamic_rnn -> (the top layer's outputs [B, T, H], [(c_l, h_l)] per layer)."""
    H = int(lstm_size)
    lengths = torch.as_tensor(lengths).reshape(-1)
    if lengths.shape[0] != inputs.shape[0]:
        raise ValueError(f"sequence_length has {lengths.shape[0]} entries for a batch of {inputs.shape[0]}")
    x, states = inputs, []
    for layer in range(int(num_layers)):
        with vs.variable_scope(f"rnn/multi_rnn_cell/cell_{layer}/basic_lstm_cell"):
            kernel = vs.get_variable("kernel", [x.shape[2] + H, 4 * H], vs.glorot_uniform_initializer(), device=inputs.device)
            bias = vs.get_variable("bias", [4 * H], vs.zeros_initializer(), device=inputs.device)
        x, h, c = lstm_layer(x, kernel, bias, lengths)
        states.append((c, h))
    return x, states


class LstmLastHiddenModule(modules.BaseModule):
    """LSTM network that outputs the last hidden state of its top layer (:20-53).  ``output_dim`` and ``scope_id`` are stored and read
    nowhere, as written."""

    def __init__(self, lstm_size, lstm_layers, num_frames, output_dim, scope_id=None):
        self.lstm_size = lstm_size
        self.lstm_layers = lstm_layers
        self.output_dim = output_dim
        self.num_frames = num_frames
        self.scope_id = scope_id

    def forward(self, inputs, **unused_params):
        """inputs [B, max_frames, F] -> [B, lstm_size]: ``state[-1].h``."""
        _, states = _stacked_lstm(inputs, self.num_frames, self.lstm_size, self.lstm_layers)
        return states[-1][1]


class LstmConcatAverageModule(modules.BaseModule):
    """LSTM layers whose result also carries the averages of the outputs and of the inputs (:56-88):
    [l2_normalize(sum_t outputs) | state | l2_normalize(sum_t inputs)], the state (state_is_tuple=False) being
    [c_0, h_0, c_1, h_1, ...] -> [B, lstm_size + 2 num_layers lstm_size + F]."""

    def __init__(self, lstm_size, num_layers, max_frame):
        self.lstm_size = lstm_size
        self.num_layers = num_layers
        self.max_frame = max_frame

    def forward(self, inputs, **unused_params):
        outputs, states = _stacked_lstm(inputs, self.max_frame, self.lstm_size, self.num_layers)
        context_memory = layers.l2_normalize(outputs.sum(dim=1), 1)                              # :84
        average_state = layers.l2_normalize(inputs.sum(dim=1), 1)                                # :85
        state = torch.cat([t for c_h in states for t in c_h], 1)
        return torch.cat([context_memory, state, average_state], 1)                              # :86
