"""MI355X-native PredictionModule: the key-point GRU of the prediction task (modules/prediction_module.py, trained by
prediction.py:97-107 and rolled out by prediction.py:116-132) on the kernels of csrc/gru.hip.

The constructor keeps the reference's `self.rnn = nn.GRU(...)` and `self.linear = nn.Linear(...)` as parameter holders, so the
same seed gives the same weights (the RNG draws come in the same order), the state_dict keys are the reference's
(`rnn.weight_ih_l0`, ..., `linear.bias`) and `.cuda()` / `load_state_dict` behave as before.  The forward pass never calls them,
with one exception: dropout between stacked layers in training mode (dropout > 0, num_layers > 1, which no shipped
configuration uses) needs nn.GRU's own dropout masks, so that case runs the reference's computation itself.

`import modules.prediction_module` resolves to this file when MNK_NATIVE_PREDICTION=1 (modules/__init__.py)."""
import torch
from torch import nn

from .gru import GRULayerFn, LinearFn, HeadFn


class PredictionModule(nn.Module):
    """
    RNN for predicting kp movement
    """

    def __init__(self, num_kp=10, kp_variance=0.01, num_features=1024, num_layers=1, dropout=0.5):
        super(PredictionModule, self).__init__()

        input_size = num_kp * (2 + 4 * (kp_variance == 'matrix'))

        self.rnn = nn.GRU(input_size=input_size, hidden_size=num_features, num_layers=num_layers,
                          dropout=dropout, batch_first=True)
        self.linear = nn.Linear(num_features, input_size)

    def _stock(self):
        return self.training and self.rnn.dropout > 0 and self.rnn.num_layers > 1

    def _rnn(self, input, h=None):
        """nn.GRU(batch_first=True)(input, h) on the native layers: (output [B, T, H], h_n [num_layers, B, H])."""
        x, hn = input, []
        for l in range(self.rnn.num_layers):
            x, h_l = GRULayerFn.apply(x, None if h is None else h[l], getattr(self.rnn, "weight_ih_l%d" % l),
                                      getattr(self.rnn, "weight_hh_l%d" % l), getattr(self.rnn, "bias_ih_l%d" % l),
                                      getattr(self.rnn, "bias_hh_l%d" % l))
            hn.append(h_l)
        return x, torch.stack(hn, 0)

    def net(self, input, h=None):
        if self._stock():
            output, h = self.rnn(input, h)
            init_shape = output.shape
            output = output.contiguous().view(-1, output.shape[-1])
            output = self.linear(output)
            return output.view(init_shape[0], init_shape[1], output.shape[-1]), h
        output, h = self._rnn(input, h)
        return LinearFn.apply(output, self.linear.weight, self.linear.bias), h

    def forward(self, kp_batch):
        bs, d, num_kp, _ = kp_batch['mean'].shape
        inputs = [kp_batch['mean'].reshape(bs, d, -1)]
        if 'var' in kp_batch:
            inputs.append(kp_batch['var'].reshape(bs, d, -1))

        input = torch.cat(inputs, dim=-1)

        output, h = self.net(input)
        if not self._stock():
            out = HeadFn.apply(output, num_kp, 'var' in kp_batch)
            return {'mean': out[0], 'var': out[1]} if 'var' in kp_batch else {'mean': out}

        output = output.view(bs, d, num_kp, -1)
        mean = torch.tanh(output[:, :, :, :2])
        kp_array = {'mean': mean}
        if 'var' in kp_batch:
            var = output[:, :, :, 2:]
            var = var.view(bs, d, num_kp, 2, 2)
            var = torch.matmul(var.permute(0, 1, 2, 4, 3), var)
            kp_array['var'] = var

        return kp_array
