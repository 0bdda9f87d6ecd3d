"""Does generated audio sound like its reference voice?  The cosine between speaker embeddings, on the device.

Host side of ``FasterQwen3TTS.speaker_similarity`` and ``python -m fq3hip.cli verify``: the clips of one call go
through ``HipRefAudioAnalyzer.speaker_embeddings`` -- one ``fq3_refenc_speaker_group`` call per 32 clips -- and one
``fq3_refenc_similarity`` launch compares them with the reference; the cosines reach the host behind one pinned copy.

No threshold is chosen here.  What cosine separates "same voice" from "another voice" depends on the checkpoint's speaker encoder and
has to be calibrated on real voices; neither was available when this was written.  Use the number to rank seeds, to log, or against
a threshold of your own.
"""
from __future__ import annotations

import os
from typing import Callable, List, Union

import numpy as np
import torch

RATE = 24000


def _is_wave_and_rate(ref) -> bool:
    return isinstance(ref, (tuple, list)) and len(ref) == 2 and np.isscalar(ref[1]) and not np.isscalar(ref[0]) and np.ndim(ref[0]) >= 1


def reference_embedding(ref):
    """The stored embedding of ``ref`` when it carries one -- a ``voice_clone_prompt`` dict, the item list ``create_voice_clone_prompt``
    returns, or a raw embedding (1-D tensor / array) -- else None: ``ref`` is audio (a path or ``(array, sr)``) and has to be analysed."""
    if isinstance(ref, dict):
        if "ref_spk_embedding" not in ref:
            raise ValueError("ref: a voice_clone_prompt needs its 'ref_spk_embedding'")
        ref = ref["ref_spk_embedding"]
        ref = ref[0] if isinstance(ref, (list, tuple)) else ref
    elif isinstance(ref, (list, tuple)) and ref and hasattr(ref[0], "ref_spk_embedding"):
        ref = ref[0].ref_spk_embedding
    elif hasattr(ref, "ref_spk_embedding"):
        ref = ref.ref_spk_embedding
    elif isinstance(ref, (str, os.PathLike)) or _is_wave_and_rate(ref):
        return None
    emb = torch.as_tensor(ref)
    if emb.dim() != 1:
        raise ValueError("ref: a path, (array, sr), a voice_clone_prompt or a 1-D speaker embedding")
    return emb


class StoredEmbedding:
    """A raw speaker embedding given where a clip is expected (``nearest_voices``): a 1-D array there is always a waveform, so an
    embedding says what it is.  ``reference_embedding`` reads it like a prompt item."""

    def __init__(self, embedding):
        self.ref_spk_embedding = embedding


def nearest_voices(analyzer, audio, sr, library, k: int = 1) -> list:
    """The ``k`` nearest voices of ``library`` (``voice_library.VoiceLibrary``) for ``audio``: one clip or a list of them, each a mono
    waveform at ``sr`` Hz (one rate or one per clip; another rate than 24 kHz goes through the device resampler), or something that
    carries its embedding, which is used as stored (``reference_embedding``): a ``voice_clone_prompt`` dict, a prompt item, or a raw
    embedding wrapped in ``StoredEmbedding``.  The waveforms share the analyser's group calls, all queries one ``library.search``.
    Returns ``[(name, cosine), ...]`` best first (a list of those for a list)."""
    one = not isinstance(audio, (list, tuple))
    clips = [audio] if one else list(audio)
    if not clips:
        return []
    rates = list(sr) if isinstance(sr, (list, tuple)) else [sr] * len(clips)
    if len(rates) != len(clips):
        raise ValueError("sr must be one rate or one per clip")
    stored = [reference_embedding(x) if isinstance(x, dict) or hasattr(x, "ref_spk_embedding") else None for x in clips]
    waves = []
    for x, r, e in zip(clips, rates, stored):
        if e is None:
            if int(r) != RATE:
                from .audio_out import resample_device
                x = resample_device(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, int(r), RATE, analyzer.device)
            waves.append(x)
    fresh = iter(analyzer.speaker_embeddings(waves)) if waves else iter(())
    q = torch.stack([next(fresh).to(analyzer.device) if e is None else e.to(device=analyzer.device, dtype=torch.float32) for e in stored])
    out = library.search(q, k)
    return out[0] if one else out


def speaker_similarity(analyzer, audio, sr, ref, reference_wave: Callable) -> Union[float, List[float]]:
    """Cosine between the speaker embedding of ``audio`` (one mono waveform or a list of them, device tensors or host arrays at ``sr``
    Hz -- one rate or one per clip) and that of ``ref``.  ``reference_wave``: what turns an audio ``ref`` into 24 kHz mono (the
    model's reference loader, host resampler).  Returns a float, or a list of floats for a list."""
    one = not isinstance(audio, (list, tuple))
    clips = [audio] if one else list(audio)
    if not clips:
        return []
    rates = list(sr) if isinstance(sr, (list, tuple)) else [sr] * len(clips)
    if len(rates) != len(clips):
        raise ValueError("sr must be one rate or one per clip")
    dev = analyzer.device
    for i, (x, r) in enumerate(zip(clips, rates)):
        if int(r) != RATE:
            from .audio_out import resample_device
            clips[i] = resample_device(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, int(r), RATE, dev)
    emb = reference_embedding(ref)
    if emb is None:                                        # the reference is audio: it rides in the same group calls as the clips
        e = analyzer.speaker_embeddings(clips + [reference_wave(ref)])
        e, emb = e[:-1], e[-1]
    else:
        e = analyzer.speaker_embeddings(clips)
        if emb.numel() != e.shape[-1]:
            raise ValueError(f"ref: an embedding of {emb.numel()} values, the speaker encoder gives {e.shape[-1]}")
    cos = analyzer.similarity(e, emb)
    host = cos
    if cos.is_cuda:
        host = torch.empty(cos.shape, dtype=torch.float32, pin_memory=True)
        host.copy_(cos, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    out = [float(v) for v in host]
    return out[0] if one else out
