"""float64 speaker encoder for clips of FEWER frames than a TDNN layer pads by, which torch's reflect padding refuses: the ECAPA-TDNN of
oracle/refenc_oracle.ecapa with the library's padding rule written out as an index -- reflect, then clamp into the clip (csrc
pad_rows_kernel, mode 0).  Where the padding is shorter than the clip the two agree; test_gpu_speaker_group.py checks that too."""
import torch
import torch.nn.functional as F

from oracle import refenc_oracle as RO


def _tdnn(W, name, x, k, dil):
    T, pad = x.shape[-1], (k - 1) * dil // 2
    if pad:
        t = torch.arange(-pad, T + pad).abs()
        t = torch.where(t >= T, 2 * (T - 1) - t, t).clamp(0, T - 1)
        x = x[..., t]
    return F.relu(F.conv1d(x, W[name + ".weight"].to(x.dtype), W[name + ".bias"].to(x.dtype), dilation=dil))


def speaker_embedding(W, rc, wav):
    h = RO.mel_spectrogram(rc, wav, torch.float64).transpose(0, 1)[None]
    S, ks, ds = "speaker_encoder", rc.enc_kernel_sizes, rc.enc_dilations
    cv = lambda n, v: F.conv1d(v, W[n + ".weight"].double(), W[n + ".bias"].double())
    x = _tdnn(W, f"{S}.blocks.0.conv", h, ks[0], ds[0])
    outs = []
    for b in range(1, len(rc.enc_channels) - 1):
        B, res, parts, prev = f"{S}.blocks.{b}", x, [], None
        for i, part in enumerate(torch.chunk(_tdnn(W, f"{B}.tdnn1.conv", x, 1, 1), rc.enc_res2net_scale, dim=1)):
            prev = part if i == 0 else _tdnn(W, f"{B}.res2net_block.blocks.{i - 1}.conv", part if i == 1 else part + prev, ks[b], ds[b])
            parts.append(prev)
        h = _tdnn(W, f"{B}.tdnn2.conv", torch.cat(parts, dim=1), 1, 1)
        gate = torch.sigmoid(cv(f"{B}.se_block.conv2", F.relu(cv(f"{B}.se_block.conv1", h.mean(dim=2, keepdim=True)))))
        x = h * gate + res
        outs.append(x)
    h = _tdnn(W, f"{S}.mfa.conv", torch.cat(outs, dim=1), ks[-1], ds[-1])
    mean = h.mean(dim=2, keepdim=True)
    std = torch.sqrt(((h - mean) ** 2).mean(dim=2, keepdim=True).clamp(1e-12))
    att = torch.tanh(_tdnn(W, f"{S}.asp.tdnn.conv", torch.cat([h, mean.expand_as(h), std.expand_as(h)], dim=1), 1, 1))
    att = torch.softmax(cv(f"{S}.asp.conv", att), dim=2)
    mean = (att * h).sum(2, keepdim=True)
    std = torch.sqrt((att * (h - mean) ** 2).sum(2, keepdim=True).clamp(1e-12))
    return cv(f"{S}.fc", torch.cat([mean, std], dim=1))[0, :, 0]
