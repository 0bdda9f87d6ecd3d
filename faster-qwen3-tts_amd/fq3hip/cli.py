#!/usr/bin/env python3
"""Command line for the MI355X path, with the reference CLI's sub-commands and flags (``faster_qwen3_tts/cli.py``):
``clone`` / ``custom`` / ``design`` synthesise one text to a WAV file, ``serve`` reads one text per stdin line
(``cli.py:228-349``).  Differences: WAV files are written with the standard library (no ``soundfile`` in this image);
``--voice-cache DIR`` serves ``--ref-audio`` from precomputed voice prompts (``fq3hip/voice_cache.py``), because
reference-audio analysis is not part of this path; ``--synthetic 0.6b|1.7b`` builds seeded random weights instead of
loading a checkpoint (smoke runs, throughput measurements); ``serve --lanes N`` decodes up to N queued lines in lock-step
(``fq3_batch_*``); ``custom`` / ``design --text-stdin`` read the text from stdin AS IT ARRIVES, line by line, and decode behind it
(``FasterQwen3TTS.stream_custom_voice`` / ``stream_voice_design``); GGML flags are accepted and refused like the wrapper refuses them."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np


def _stream_to_audio(gen):
    chunks, sr = [], None
    for audio_chunk, sr, _ in gen:
        chunks.append(audio_chunk)
    if not chunks:
        return np.zeros(1, dtype=np.float32), 24000
    return np.concatenate(chunks), sr


def load_model(args):
    """``cli.py:14-45``."""
    import torch
    from .model import FasterQwen3TTS
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}.get(args.dtype)
    if dtype is None:
        raise SystemExit("ERROR: --dtype fp16 is not built on this path (bf16 or fp32)")
    if args.backend != "torch":
        return FasterQwen3TTS.from_pretrained(args.model, backend=args.backend)       # raises NotImplementedError, as documented
    if args.synthetic:
        from .config import qwen3_tts_0p6b, qwen3_tts_1p7b
        from .weights import synth_weights
        cfg = qwen3_tts_0p6b() if args.synthetic == "0.6b" else qwen3_tts_1p7b()
        cfg.spk_id = {"synthetic": cfg.talker.vocab_size - 1024 + 300}
        cfg.spk_is_dialect = {"synthetic": False}
        W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "codec", "text"), codec_normalized=True)
        model = FasterQwen3TTS.from_weights(cfg, W, device=args.device, dtype=dtype, max_seq_len=2048)
    else:
        model = FasterQwen3TTS.from_pretrained(args.model, device=args.device, dtype=dtype, attn_implementation="sdpa",
                                               max_seq_len=2048)
    if getattr(args, "voice_cache", None):
        model.set_voice_ref_cache(args.voice_cache)
    if int(getattr(args, "prefix_cache_rows", 0) or 0) > 0:
        model.enable_prefix_cache(int(args.prefix_cache_rows))
    return model


def validate_clone_refs(args):
    """``cli.py:63-78`` (the cached-reference flags belong to the GGML backend there; here --voice-cache plays that role)."""
    if args.ref_spk or args.ref_rvq:
        print("ERROR: --ref-spk/--ref-rvq belong to the GGML backend; use --voice-cache DIR with --ref-audio")
        sys.exit(2)
    if not args.ref_audio:
        print("ERROR: clone mode requires --ref-audio")
        sys.exit(2)
    if not args.xvec_only and not args.ref_text and not args.voice_cache:
        print("ERROR: --ref-text is required with --ref-audio unless --xvec-only is set")
        sys.exit(2)


def _gen_kwargs(args):
    return dict(max_new_tokens=args.max_new_tokens, temperature=args.temperature, top_k=args.top_k, do_sample=not args.greedy,
                repetition_penalty=args.repetition_penalty)


def _stdin_pieces(lines=None):
    """Lines as they arrive (``readline``: iterating a pipe would wait for a full read-ahead buffer)."""
    if lines is not None:
        yield from lines
        return
    while True:
        line = sys.stdin.readline()
        if not line:
            return
        yield line


def synthesize_text_stream(model, args, pieces):
    """``--text-stdin``: the text is fed while it arrives -> (waveform, sample_rate)."""
    kw = dict(chunk_size=args.chunk_size, **_gen_kwargs(args))
    if args.mode == "custom":
        return _stream_to_audio(model.stream_custom_voice(pieces, speaker=args.speaker, language=args.language, instruct=args.instruct, **kw))
    return _stream_to_audio(model.stream_voice_design(pieces, instruct=args.instruct, language=args.language, **kw))


def synthesize(model, args, text: str):
    """One text -> (waveform, sample_rate) in the selected mode (``cli.py:81-225``)."""
    kw = _gen_kwargs(args)
    if getattr(args, "long", False) and args.mode in ("clone", "custom"):
        from .long_form import LongFormSpec
        lkw = dict(lanes=args.lanes, long_form=LongFormSpec(max_chars=args.max_chars), **kw)
        if args.mode == "clone":
            lkw.update(text=text, language=args.language, ref_audio=args.ref_audio, ref_text=args.ref_text, xvec_only=args.xvec_only,
                       non_streaming_mode=args.non_streaming_mode)
            name = "generate_long_voice_clone"
        else:
            lkw.update(text=text, speaker=args.speaker, language=args.language, instruct=args.instruct)
            name = "generate_long_custom_voice"
        if args.streaming:
            return _stream_to_audio(getattr(model, name + "_streaming")(chunk_size=args.chunk_size, **lkw))
        audio_list, sr = getattr(model, name)(**lkw)
        return audio_list[0], sr
    if args.mode == "clone":
        ckw = dict(text=text, language=args.language, ref_audio=args.ref_audio, ref_text=args.ref_text, xvec_only=args.xvec_only,
                   non_streaming_mode=args.non_streaming_mode, **kw)
        if args.streaming:
            return _stream_to_audio(model.generate_voice_clone_streaming(chunk_size=args.chunk_size, **ckw))
        audio_list, sr = model.generate_voice_clone(**ckw)
        return audio_list[0], sr
    if args.mode == "custom":
        ckw = dict(text=text, speaker=args.speaker, language=args.language, instruct=args.instruct, **kw)
        if args.streaming:
            return _stream_to_audio(model.generate_custom_voice_streaming(chunk_size=args.chunk_size, **ckw))
        audio_list, sr = model.generate_custom_voice(**ckw)
        return audio_list[0], sr
    ckw = dict(text=text, instruct=args.instruct, language=args.language, **kw)
    if args.streaming:
        return _stream_to_audio(model.generate_voice_design_streaming(chunk_size=args.chunk_size, **ckw))
    audio_list, sr = model.generate_voice_design(**ckw)
    return audio_list[0], sr


def _output_stage(model, args):
    """``--out-rate`` / ``--encoding`` / ``--speed``: the model's ``audio_output`` context (time-scaling, resampling and encoding on
    the device), or a no-op."""
    import contextlib
    rate, enc, speed = getattr(args, "out_rate", None), getattr(args, "encoding", None), getattr(args, "speed", None)
    if rate is None and enc is None and speed is None:
        return contextlib.nullcontext()
    return model.audio_output(rate, enc or "f32", 1.0 if speed is None else speed)


def _output_spec(args):
    """``--out-rate`` / ``--encoding`` / ``--speed`` as the ``output=`` of the batch entry points: an ``AudioOutSpec``, or None."""
    rate, enc, speed = getattr(args, "out_rate", None), getattr(args, "encoding", None), getattr(args, "speed", None)
    if rate is None and enc is None and speed is None:
        return None
    from .audio_out import AudioOutSpec
    return AudioOutSpec(rate, enc or "f32", 1.0 if speed is None else speed)


def _seeded(model, args):
    """``--seed``: the model's ``seeded`` context, or a no-op."""
    import contextlib
    seed = getattr(args, "seed", None)
    return contextlib.nullcontext() if seed is None else model.seeded(seed)


def _exact(model, args):
    """``--exact-streaming``: the model's ``exact_streaming`` context, or a no-op."""
    import contextlib
    return model.exact_streaming() if getattr(args, "exact_streaming", False) else contextlib.nullcontext()


def _levelled(model, args):
    """``--loudness`` / ``--gain-db``: the model's ``loudness`` or ``fixed_gain`` context (the level set on the device), or a no-op;
    ``--level``: the model's ``leveller`` context (the streaming loudness leveller, behind the gain);
    ``--limiter-db``: the model's ``limiter`` context around it (the limiter runs behind the gain and the leveller)."""
    import contextlib
    lufs, gain, ceiling = getattr(args, "loudness", None), getattr(args, "gain_db", None), getattr(args, "limiter_db", None)
    stack = contextlib.ExitStack()
    if lufs is not None:
        stack.enter_context(model.loudness(target_lufs=lufs))
    elif gain is not None:
        stack.enter_context(model.fixed_gain(gain))
    if getattr(args, "level", None) is not None:
        stack.enter_context(model.leveller(target_lufs=args.level))
    if ceiling is not None:
        stack.enter_context(model.limiter(ceiling_db=ceiling))
    return stack


def check_level_args(parser, args):
    """``--loudness`` needs the whole utterance: an argparse error together with a streaming mode or with ``--gain-db``; so is a
    ``--loudness`` or ``--gain-db`` outside its range (said before the model is loaded)."""
    from .loudness import LoudnessSpec, gain_factor
    try:
        if getattr(args, "loudness", None) is not None:
            LoudnessSpec(target_lufs=args.loudness)
        if getattr(args, "gain_db", None) is not None:
            gain_factor(args.gain_db)
        if getattr(args, "limiter_db", None) is not None:
            from .limiter import LimiterSpec
            LimiterSpec(ceiling_db=args.limiter_db)
        if getattr(args, "level", None) is not None:
            from .leveller import LevelSpec
            LevelSpec(target_lufs=args.level)
    except ValueError as exc:
        parser.error(str(exc))
    if getattr(args, "loudness", None) is None:
        return
    if getattr(args, "level", None) is not None:
        parser.error("--loudness and --level answer the same question: give one (--level also works on a stream)")
    if getattr(args, "streaming", False) or getattr(args, "text_stdin", False):
        parser.error("--loudness measures the whole utterance, so it does not go with --streaming / --text-stdin: a stream's gain cannot "
                     "be known before it ends (use --gain-db X)")
    if getattr(args, "gain_db", None) is not None:
        parser.error("--loudness and --gain-db both set the level: give one")


def _write_output(path, audio, sr, args):
    """float32 audio as 16-bit PCM (as ever); what the output stage encoded (int16, G.711 bytes, a FLAC stream) as it is."""
    import os
    from .audio_io import write_wav, write_wav_encoded
    enc = getattr(args, "encoding", None)
    if enc == "flac":
        if not path.lower().endswith(".flac"):
            print(f"WARNING: {path} receives a FLAC stream; a .flac name would say so")
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(audio, dtype=np.uint8).tobytes())
    elif enc in ("s16", "mulaw", "alaw"):
        write_wav_encoded(path, audio, sr, enc)
    else:
        write_wav(path, audio, sr)


def _check_mode_args(args):
    if args.mode == "clone":
        validate_clone_refs(args)
    if args.mode == "custom" and not args.speaker:
        print("ERROR: --speaker is required for custom mode")
        sys.exit(2)
    if args.mode == "design" and not args.instruct:
        print("ERROR: --instruct is required for design mode")
        sys.exit(2)


def cmd_once(args, model=None, lines=None):
    from .audio_io import write_wav
    _check_mode_args(args)
    text_stdin = bool(getattr(args, "text_stdin", False))
    if text_stdin == (args.text is not None):
        print("ERROR: give either --text or --text-stdin")
        sys.exit(2)
    model = model or load_model(args)
    start = time.perf_counter()
    with _levelled(model, args), _output_stage(model, args), _seeded(model, args), _exact(model, args):
        audio, sr = synthesize_text_stream(model, args, _stdin_pieces(lines)) if text_stdin else synthesize(model, args, args.text)
    total = time.perf_counter() - start
    _write_output(args.output, audio, sr, args)
    if getattr(args, "encoding", None) == "flac":              # bytes, not samples: the duration is inside the stream
        print(f"Wrote {args.output} ({len(audio)} bytes of FLAC in {total:.2f}s)")
        return
    dur = len(audio) / sr if sr else 0.0
    print(f"Wrote {args.output} (dur {dur:.2f}s, RTF {dur / total if total > 0 else 0.0:.2f})")


def cmd_serve(args, model=None, lines=None):
    """``cli.py:228-349``: one text per input line -> ``out_NNNN.wav``.  With ``--lanes N > 1`` (clone mode) the lines that are
    already waiting are decoded together, up to N in lock-step over one weight stream."""
    import os
    from .audio_io import write_wav
    _check_mode_args(args)
    model = model or load_model(args)
    print("Server started. Enter text per line. Type 'exit' or 'quit' to stop.")
    idx = 1
    it = iter(lines if lines is not None else sys.stdin)
    pending, stop = [], False
    while not stop:
        pending.clear()
        for line in it:
            text = line.strip()
            if not text:
                continue
            if text.lower() in ("exit", "quit", "stop"):
                stop = True
                break
            pending.append(text)
            if len(pending) >= max(1, args.lanes) or args.lanes <= 1:
                break
        else:
            stop = True
        if not pending:
            continue
        start = time.perf_counter()
        levelled = any(getattr(args, k, None) is not None for k in ("gain_db", "limiter_db", "level"))
        if len(pending) > 1 and getattr(args, "long", False) and args.mode in ("clone", "custom") and not levelled:
            # --long: every line is a text of any length; the segments of all waiting lines share the lanes of ONE lock-step run
            from .long_form import LongFormSpec
            spec = _output_spec(args)
            lkw = dict(lanes=args.lanes, long_form=LongFormSpec(max_chars=args.max_chars), seeds=getattr(args, "seed", None),
                       **_gen_kwargs(args), **({} if spec is None else dict(output=spec)))
            if args.mode == "clone":
                results = model.generate_long_voice_clone_batch(pending, language=args.language, ref_audio=args.ref_audio,
                                                                ref_text=args.ref_text, xvec_only=args.xvec_only,
                                                                non_streaming_mode=args.non_streaming_mode, **lkw)
            else:
                results = model.generate_long_custom_voice_batch(pending, speaker=args.speaker, language=args.language,
                                                                 instruct=args.instruct, **lkw)
            outs = [(r[0][0], r[1]) for r in results]
        elif len(pending) > 1 and args.mode == "clone" and not levelled:    # (--gain-db / --limiter-db: line by line, as before)
            # --out-rate / --encoding / --speed: the lines decoded together go through the output stage together (``output=``)
            spec = _output_spec(args)
            results = model.generate_voice_clone_batch(pending, language=args.language, ref_audio=args.ref_audio, ref_text=args.ref_text,
                                                       xvec_only=args.xvec_only, non_streaming_mode=args.non_streaming_mode,
                                                       lanes=args.lanes, **_gen_kwargs(args), **({} if spec is None else dict(output=spec)))
            outs = [(r[0][0], r[1]) for r in results]
        else:
            with _levelled(model, args), _output_stage(model, args), _exact(model, args):
                outs = [synthesize(model, args, t) for t in pending]
        total = time.perf_counter() - start
        for audio, sr in outs:
            flac = getattr(args, "encoding", None) == "flac"
            out_path = os.path.join(args.output_dir, f"out_{idx:04d}.{'flac' if flac else 'wav'}")
            idx += 1
            _write_output(out_path, audio, sr, args)
            if flac:
                print(f"Wrote {out_path} ({len(audio)} bytes of FLAC)")
                continue
            dur = len(audio) / sr if sr else 0.0
            print(f"Wrote {out_path} (dur {dur:.2f}s, RTF {dur * len(outs) / total if total > 0 else 0.0:.2f})")


def build_parser():
    p = argparse.ArgumentParser(prog="faster-qwen3-tts", description="FasterQwen3TTS CLI (MI355X HIP path)")
    p.add_argument("--device", default="cuda", help="Device (a ROCm GPU: 'cuda' in PyTorch-ROCm)")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"], help="Model dtype")
    p.add_argument("--backend", default="torch", choices=["torch", "ggml"], help="Inference backend ('ggml' is refused on this path)")
    p.add_argument("--synthetic", choices=["0.6b", "1.7b"], help="seeded random weights at the real shapes instead of a checkpoint")
    p.add_argument("--voice-cache", help="directory of precomputed voice prompts (<key>.spk/.rvq/.json) serving --ref-audio")
    sub = p.add_subparsers(dest="command", required=True)

    def common(sp, output=True, text_stdin=False):
        sp.add_argument("--model", default="Qwen/Qwen3-TTS-12Hz-0.6B-Base", help="local checkpoint directory")
        sp.add_argument("--language", default="English")
        sp.add_argument("--max-new-tokens", type=int, default=2048)
        sp.add_argument("--temperature", type=float, default=0.9)
        sp.add_argument("--top-k", type=int, default=50)
        sp.add_argument("--repetition-penalty", type=float, default=1.05)
        sp.add_argument("--greedy", action="store_true")
        sp.add_argument("--streaming", action="store_true")
        sp.add_argument("--chunk-size", type=int, default=12)
        sp.add_argument("--exact-streaming", action="store_true",
                        help="with --streaming: the streamed audio is the one-pass decode of the codes, whatever --chunk-size "
                             "(default: the reference's 25-frame windowing)")
        sp.add_argument("--out-rate", type=int, default=None, metavar="HZ",
                        help="output sample rate, resampled on the device (e.g. 8000, 16000, 44100, 48000; default: the model's)")
        sp.add_argument("--encoding", default=None, choices=["f32", "s16", "mulaw", "alaw", "flac"],
                        help="sample encoding done on the device; mulaw / alaw write a G.711 WAV, flac a FLAC file of the s16 samples, "
                             "compressed on the device (default: float32, written as 16-bit)")
        sp.add_argument("--speed", type=float, default=None, metavar="X",
                        help="speaking rate, 0.25 to 4.0, time-scaled on the device: duration changes, pitch does not (default: 1.0)")
        sp.add_argument("--gain-db", type=float, default=None, metavar="X",
                        help="multiply the audio by 10^(X/20) on the device, in front of --speed / --out-rate / --encoding; no limiter "
                             "(default: off)")
        sp.add_argument("--limiter-db", type=float, default=None, metavar="DB",
                        help="true-peak look-ahead limiter on the device behind the gain: no sample leaves above DB dBFS (-20 to 0; 5 ms "
                             "look-ahead, 20 ms hold); works in every mode, streaming included (default: off)")
        sp.add_argument("--level", type=float, default=None, metavar="LUFS",
                        help="streaming loudness leveller on the device: a causal BS.1770 gain that brings the stream to LUFS while it "
                             "runs (zero latency, at most +20 dB); works in every mode, streaming included; it does not limit, so add "
                             "--limiter-db; the defaults behind it are not tuned on real voices (default: off)")
        if output:
            sp.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                            help="measure the utterance on the device (ITU-R BS.1770-4, integrated) and scale it to LUFS, at most +20 dB and "
                                 "a sample peak of -1 dBFS; with --long every segment is levelled on its own; not with a streaming mode")
            sp.add_argument("--seed", type=int, default=None, metavar="N",
                            help="sampling seed in [0, 2^64): the same command gives the same audio (default: unseeded)")
            sp.add_argument("--text", required=not text_stdin)
            if text_stdin:
                sp.add_argument("--text-stdin", action="store_true",
                                help="read the text from stdin as it arrives (line by line) and decode behind it "
                                     "(one stream; many streams at once: the server's /v1/audio/speech/sessions)")
            sp.add_argument("--output", required=True)

    def clone_refs(sp):
        sp.add_argument("--ref-audio")
        sp.add_argument("--ref-text", default="")
        sp.add_argument("--ref-spk")
        sp.add_argument("--ref-rvq")
        sp.add_argument("--xvec-only", action="store_true")
        sp.add_argument("--non-streaming-mode", action="store_true", default=None)

    def prefix_cache_flag(sp):
        sp.add_argument("--prefix-cache-rows", type=int, default=0, metavar="N",
                        help="keep the talker K/V rows of instruct turns on the device, up to N rows, and prefill only the rest of a "
                             "prompt whose instruct is cached (default 0: off; the server honours it under both schedulers)")

    def long_form_flags(sp):
        sp.add_argument("--long", action="store_true",
                        help="long form: cut the text into segments, decode them side by side and join them on the device into one stream")
        sp.add_argument("--max-chars", type=int, default=240, metavar="N", help="--long: the splitter's budget per segment")
        sp.add_argument("--lanes", type=int, default=16, metavar="N", help="--long: segments decoded side by side")

    c = sub.add_parser("clone", help="voice cloning from reference audio")
    common(c); clone_refs(c); long_form_flags(c); c.set_defaults(mode="clone", func=cmd_once)
    c = sub.add_parser("custom", help="CustomVoice model: predefined speaker")
    common(c, text_stdin=True); c.add_argument("--speaker"); c.add_argument("--instruct"); c.set_defaults(mode="custom", func=cmd_once)
    prefix_cache_flag(c); long_form_flags(c)
    c = sub.add_parser("design", help="VoiceDesign model: voice from an instruction")
    common(c, text_stdin=True); c.add_argument("--instruct"); c.set_defaults(mode="design", func=cmd_once)
    prefix_cache_flag(c)
    s = sub.add_parser("serve", help="read one text per stdin line, write out_NNNN.wav")
    common(s, output=False); clone_refs(s)
    s.add_argument("--mode", default="clone", choices=["clone", "custom", "design"])
    s.add_argument("--speaker"); s.add_argument("--instruct")
    s.add_argument("--output-dir", default="outputs")
    s.add_argument("--lanes", type=int, default=1, help="decode up to N waiting lines in lock-step (clone mode)")
    s.add_argument("--long", action="store_true",
                   help="every line is a text of any length (long form): with --lanes N the segments of up to N waiting lines share "
                        "the N lanes of one lock-step run (clone and custom mode)")
    s.add_argument("--max-chars", type=int, default=240, metavar="N", help="--long: the splitter's budget per segment")
    s.set_defaults(func=cmd_serve)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_level_args(parser, args)
    args.func(args)


if __name__ == "__main__":
    main()
