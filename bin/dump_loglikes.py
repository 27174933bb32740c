#!/usr/bin/env python
"""Writes the acoustic model's log-likelihoods (logits - log prior) of a set of utterances to a Kaldi matrix
archive -- command line of the reference's bin/dump_loglikes.py (same flags; the archive is what Kaldi's
latgen-faster-mapped reads), running on libpk2hip.so: fbank + CMN + BLSTM forward on the device.

  python bin/dump_loglikes.py -config configs/ce.yaml -model_path exp/ce/model.ce.0.tar -data_path dev.zip \
      -prior_path exp/tri/final.occs -out_file exp/ce/loglikes.ark

Checkpoints of the reference's NnetAM(LSTMStack) (keys `nnet.lstm.*`) and of LSTMAM (`lstm.*`), with or without
DataParallel's `module.` prefix, load unchanged.  -synthetic draws seeded utterances and uses uniform priors.
-array_frontend mvdr | wpe_mvdr reads every channel of the recordings (the 7-channel LibriCSS evaluation) and puts each
utterance through (WPE ->) cGMM masks -> MVDR on the device before the filterbank (pykaldi2_amd.cgmm.ArrayFrontEnd); with
-synthetic the utterances are first recorded by a simulated 7-microphone array.  -array_frontend sep_mvdr | wpe_sep_mvdr
separates overlapped speech instead (pykaldi2_amd.separate: blind cGMM masks aligned over the bins, one MVDR per speaker):
every recording writes one matrix per stream under the keys <utt>_s0 .. <utt>_s{S-1}, S = -num_speakers; with -synthetic
the recording is the utterance overlapped by a second seeded one in the same simulated room.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch as th
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import cgmm, data, fbank, kaldi_io, lstm, se  # noqa: E402


def synthetic_array(wav, index, dev, overlap=False):
    """A seeded 7-channel recording of a synthetic utterance, so that -array_frontend runs without data: the utterance and
    a directional noise in a sampled room (rirgen, the circular array of beamform.array_geometry()), mixed by
    MultiSourceSimulator.  overlap=True (the separating front ends): the second position of the same room holds a second
    seeded utterance instead of the noise, and the mixer places the two as overlapping sources.  (C, n) CUDA float32, n the
    utterance's length; numpy's generator is left as it was."""
    from pykaldi2_amd import _lib, beamform, rirgen, simulation, synth
    state = np.random.get_state()
    np.random.seed(20161 + index)
    try:
        room, t60, mic, src = rirgen.sample_online_room((0.1, 0.5), 2, mic_positions=beamform.array_geometry())
        b = rirgen.rirgen_batch([dict(room=room, source_loc=src, mic_loc=mic, t60=t60)], device=dev)
        rirs, dl = b.rirs[0], b.delays[0]
        if overlap:
            other = np.ascontiguousarray(synth.waveform(np.random.default_rng(977 + index), wav.shape[0] / 16000.0), np.float32)
            sim = simulation.MultiSourceSimulator(use_rir=True, use_noise=False, n_source_range=(2, 2))
            mixed = sim([_lib.h2d(wav, dev), _lib.h2d(other, dev)], None, [rirs[0], rirs[1]], None, rir_delays=[dl[0], dl[1]])[0]
        else:
            noise = np.ascontiguousarray(synth.waveform(np.random.default_rng(977 + index), wav.shape[0] / 16000.0 + 0.5),
                                         np.float32)
            sim = simulation.MultiSourceSimulator(use_rir=True, use_noise=True, n_source_range=(1, 1))
            mixed = sim([_lib.h2d(wav, dev)], [_lib.h2d(noise, dev)], [rirs[0]], [rirs[1]], rir_delays=[dl[0], dl[1]])[0]
    finally:
        np.random.set_state(state)
    n = wav.shape[0]
    if mixed.shape[1] < n:
        mixed = th.nn.functional.pad(mixed, (0, n - mixed.shape[1]))
    return mixed[:, :n].contiguous()


def enhance(frontend, arrays, dev):
    """arrays: host or device (C, n) signals of one batch -> list of device float32 (n,): the array front end on the
    utterances with more than one channel, grouped by their channel count (one launch per stage and group); a
    one-channel signal passes through.  A separating front end gives a list of waveforms per signal."""
    arrays = [a if isinstance(a, th.Tensor) else th.from_numpy(a).to(dev) for a in arrays]
    out = [None] * len(arrays)
    for C in sorted(set(a.shape[0] for a in arrays)):
        idx = [i for i, a in enumerate(arrays) if a.shape[0] == C]
        for i, y in zip(idx, frontend([arrays[i] for i in idx])):
            out[i] = y
    return out


def arg_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-config")
    parser.add_argument("-model_path")
    parser.add_argument("-data_path")
    parser.add_argument("-prior_path", help="the path to load the final.occs file")
    parser.add_argument("-transform", help="feature transformation matrix or mvn statistics")
    parser.add_argument("-out_file", help="write out the log-probs to this file")
    parser.add_argument("-batch_size", default=32, type=int, help="Override the batch size in the config")
    parser.add_argument("-sweep_size", default=200, type=float, help="process n hours of data per sweep (default:60)")
    parser.add_argument("-data_loader_threads", default=4, type=int, help="number of workers for data loading")
    parser.add_argument("-frame_subsampling_factor", default=1, type=int, help="the factor to subsample the features (decode.py)")
    parser.add_argument("-gpuid", default=0, type=int, help="GPU ID (decode.py)")
    parser.add_argument("-synthetic", type=int, default=0, help="dump this many seeded synthetic utterances instead")
    parser.add_argument("-array_frontend", default="none", choices=list(cgmm.FRONT_ENDS),
                        help="multi-channel front end in front of the filterbank: mvdr (cGMM masks -> MVDR) or wpe_mvdr (WPE "
                             "first); sep_mvdr | wpe_sep_mvdr: blind separation, one stream per speaker under the keys "
                             "<utt>_s0 ...; every channel of a WAV is read (default none: channel 0)")
    parser.add_argument("-num_speakers", default=2, type=int,
                        help="streams per recording of -array_frontend sep_mvdr | wpe_sep_mvdr (default 2)")
    return parser


def main():
    args = arg_parser().parse_args()

    with open(args.config) as f:
        config = yaml.safe_load(f)
    config["sweep_size"] = args.sweep_size
    print("job starts with config {}".format(json.dumps(config, sort_keys=True, indent=4)))
    dev = th.device("cuda", args.gpuid)
    th.cuda.set_device(dev)
    mc = config["model_config"]
    P = mc["label_size"]
    model = lstm.LSTMAM(mc["feat_dim"], P, mc["hidden_size"], mc["num_layers"], mc["dropout"], True).to(dev)
    if args.model_path:
        assert os.path.isfile(args.model_path), "ERROR: model file {} does not exit!".format(args.model_path)
        sd = th.load(args.model_path, map_location="cpu")["model"]
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        sd = {(k[5:] if k.startswith("nnet.") else k): v for k, v in sd.items()}   # NnetAM(LSTMStack) -> LSTMAM keys
        model.load_state_dict(sd)
        print("=> loaded checkpoint '{}' ".format(args.model_path))
    if args.prior_path:
        log_prior = se.log_prior_from_counts(se.read_kaldi_vector(args.prior_path)).to(dev)
    else:
        log_prior = se.log_prior_from_counts(np.ones(P)).to(dev)
    transform = None
    if args.transform and os.path.isfile(args.transform):
        transform = fbank.GlobalMeanVarianceNormalization.load(args.transform)
    separates = args.array_frontend in ("sep_mvdr", "wpe_sep_mvdr")
    frontend = None
    if args.array_frontend != "none":
        frontend = cgmm.ArrayFrontEnd(args.array_frontend, **(dict(num_speakers=args.num_speakers) if separates else {}))
    if args.synthetic:
        source = data.SyntheticSource(P, seed=11)
        utts = [source.draw() for _ in range(args.synthetic)]
        if frontend:
            utts = [(synthetic_array(u[0], i, dev, overlap=separates),) + tuple(u[1:]) for i, u in enumerate(utts)]
    elif frontend:
        source = data.ZipWavSource([dict(wav=args.data_path)])
        utts = []
        for z, m, u, _, _ in source.items:
            source._read(z, m)                        # opens the archive and checks the rate
            utts.append((data.decode_wav_channels(source._zips[z].read(m))[0], None, None, u))
        if any(u[0].shape[0] == 1 for u in utts):
            import warnings
            warnings.warn("-array_frontend %s: %d of %d files have one channel and pass through as they are"
                          % (args.array_frontend, sum(u[0].shape[0] == 1 for u in utts), len(utts)))
    else:
        source = data.ZipWavSource([dict(wav=args.data_path)])
        utts = [(source._read(z, m), None, None, u) for z, m, u, _, _ in source.items]
    fb = fbank.FbankExtractor()
    model.eval()
    n_batches = (len(utts) + args.batch_size - 1) // args.batch_size
    with th.no_grad(), kaldi_io.MatrixWriter("ark:" + args.out_file) as llout:
        for i in range(n_batches):
            chunk = utts[i * args.batch_size:(i + 1) * args.batch_size]
            keys = [u[3] for u in chunk]
            if frontend:
                waves = enhance(frontend, [u[0] for u in chunk], dev)
                if separates:      # one matrix per stream; a one-channel file came back once and keeps its key
                    keys = [k if u[0].shape[0] == 1 else "%s_s%d" % (k, s) for k, u, st in zip(keys, chunk, waves)
                            for s in range(len(st))]
                    waves = [w for st in waves for w in st]
                lens = [int(w.shape[0]) for w in waves]
                wav = th.cat(waves)
            else:
                lens = [u[0].shape[0] for u in chunk]
                wav = th.from_numpy(np.concatenate([u[0] for u in chunk])).to(dev)
            feats, frames, row_off = fb(wav, lens)
            if transform is not None:
                feats = transform(feats)
            sub = max(1, args.frame_subsampling_factor)          # reference decode.py:108-110: every sub-th frame, T // sub frames
            x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=sub, time_major=True)
            if sub > 1:
                frames = [int(t) // sub for t in frames]
            prediction = model.forward_time_major(x).transpose(0, 1)
            # save only the unpadded part of each utterance in the batch
            for j in range(len(keys)):
                llout[keys[j]] = prediction[j, :frames[j], :] - log_prior
            print("Process batch [{}/{}]".format(i + 1, n_batches))


if __name__ == '__main__':
    main()
