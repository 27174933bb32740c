#!/usr/bin/env python
"""Sequence-discriminative training with alignments made on the fly -- command line of the reference's bin/train_se2.py
(same flags, same YAML schema, same checkpoint format model.se.{epoch}.tar), running on libpk2hip.so.

  python bin/train_se2.py -config configs/se.yaml -data configs/data.yaml -exp_dir exp/se2 -criterion mmi \
      -seed_model exp/ce/model.ce.0.tar -trans_model exp/tri -lang_dir data/lang -prior_path exp/tri/final.occs \
      -den_dir exp/tri/graph -lr 1e-5 -batch_size 8

Unlike train_se.py, the label files' `aux_label` holds each utterance's word ids, and the numerator alignment is made
from them with the current model (reference :256-273): one pykaldi2_amd.chain.MappedAligner.align_batch per minibatch
aligns prediction - log_prior on the device (training graphs from <trans_model>/final.mdl, <trans_model>/tree,
<lang_dir>/L.fst and <lang_dir>/phones/disambig.int; beam = decoder_config.align_beam, transition_scale 1.0,
self_loop_scale 0.1, acoustic_scale 0.1 as in the reference).  An utterance that fails to align is left out of the
sequence term.  The lattices, criteria and optimiser are train_se.py's.  -criterion mwe trains with N-best minimum word
error (ops.MWEBatchFunction) against the word transcript, or with `phone_level: true` against the phones of the on-the-fly
alignment; its settings come from an optional `mwe_config:` block of the YAML (pykaldi2_amd.se.mwe_settings: num_paths 16,
lm_weight 1.0, am_weight = decoder_config.acoustic_scale, equal_weight / phone_level / distinct false).
-criterion ts distils a teacher into the model over the teacher's lattices (ops.TeacherStudentBatch: the lattices are decoded
from the teacher's log-likelihoods and rescored with the model's); -teacher_model PATH is the teacher's checkpoint, an optional
`teacher_config:` block of the YAML overrides `model_config` keys for it (a teacher of another size), and `ts_config:
{lm_weight, am_weight, old_acoustic_scale}` (pykaldi2_amd.se.ts_settings: 1.0, decoder_config.acoustic_scale, 0.0) sets the
lattice scales.  The transcripts are not used.

  python bin/train_se2.py -config configs/se.yaml -data configs/data.yaml -exp_dir exp/ts -criterion ts \
      -seed_model exp/ce/model.ce.0.tar -teacher_model exp/big/model.se.0.tar -trans_model exp/tri -lang_dir data/lang \
      -prior_path exp/tri/final.occs -den_dir exp/tri/graph -lr 1e-5 -batch_size 8

-synthetic trains on seeded generators: the word-loop HCLG of train_se.py, the L.fst of its pronunciations (pykaldi2_amd.synth.lexicon_arcs), a monophone tree and
random word transcripts short enough for their utterances.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch as th
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import augment, beamform, chain, data, dereverb, fbank, hvd, lattice, lstm, ops, optim, se, synth, utils  # noqa: E402


def parse_config(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-config")
    parser.add_argument("-data", help="data yaml file")
    parser.add_argument("-dataPath", default='', type=str, help="path of data files")
    parser.add_argument("-seed_model", default='', help="the seed nerual network model")
    parser.add_argument("-exp_dir", help="the directory to save the outputs")
    parser.add_argument("-teacher_model", default='', help="(-criterion ts) the teacher's checkpoint")
    parser.add_argument("-transform", help="feature transformation matrix or mvn statistics")
    parser.add_argument("-criterion", type=str, choices=["mmi", "mpfe", "smbr", "mwe", "ts"], default="mmi",
                        help="set the sequence training crtierion")
    parser.add_argument("-trans_model", help="the HMM transistion model directory")
    parser.add_argument("-prior_path", help="the prior for decoder, usually named as final.occs in kaldi setup")
    parser.add_argument("-den_dir", help="the decoding graph directory to find HCLG and words.txt files")
    parser.add_argument("-lang_dir", help="the lexicon directory to find L.fst")
    parser.add_argument("-lr", type=float, default=1e-5, help="set the learning rate")
    parser.add_argument("-ce_ratio", default=0.1, type=float, help="the ratio for ce regularization")
    parser.add_argument("-momentum", default=0, type=float, help="set the momentum")
    parser.add_argument("-weight_decay", default=1e-4, type=float, help="set the L2 regularization weight")
    parser.add_argument("-batch_size", default=32, type=int, help="Override the batch size in the config")
    parser.add_argument("-data_loader_threads", default=0, type=int, help="number of workers for data loading")
    parser.add_argument("-max_grad_norm", default=5, type=float, help="max_grad_norm for gradient clipping")
    parser.add_argument("-sweep_size", default=100, type=float, help="process n hours of data per sweep (default:100)")
    parser.add_argument("-num_epochs", default=1, type=int, help="number of training epochs (default:1)")
    parser.add_argument('-print_freq', default=10, type=int, metavar='N', help='print frequency (default: 10)')
    parser.add_argument('-save_freq', default=1000, type=int, metavar='N', help='save model frequency (default: 1000)')
    parser.add_argument('-synthetic', action='store_true', help='seeded synthetic utterances, HCLG, lexicon and models')
    parser.add_argument('-graph_words', default=2000, type=int, help='(synthetic) vocabulary of the word-loop HCLG')
    args = parser.parse_args(argv)
    with open(args.config) as f:
        config = yaml.safe_load(f)
    if args.data and not args.synthetic:
        with open(args.data) as f:
            d = yaml.safe_load(f)
            config["source_paths"] = [j for i, j in d['clean_source'].items()]
            if 'dir_noise' in d:
                config["dir_noise_paths"] = [j for i, j in d['dir_noise'].items()]
            if 'rir' in d:
                config["rir_paths"] = [j for i, j in d['rir'].items()]
    config['data_path'] = args.dataPath
    config["sweep_size"] = args.sweep_size
    config["synthetic"] = args.synthetic
    print("pytorch version:{}".format(th.__version__))
    print("Experiment starts with config {}".format(json.dumps(config, sort_keys=True, indent=4)))
    return args, config


def main():
    args, config = parse_config()
    augment.refuse_speed_perturb(config, "train_se2.py")     # frame-level labels: exits before a model is built
    augment.refuse_time_warp(config, "train_se2.py")
    args.spec = augment.SpecAugment.from_config(config)      # None without data_config spec_augment
    beamform.require_beamform_config(config, os.path.basename(sys.argv[0]))      # data_config beamform needs online_rir
    dereverb.require_wpe_config(config, os.path.basename(sys.argv[0]))           # data_config wpe needs use_reverb
    hvd.init()
    th.cuda.set_device(hvd.local_rank())
    dev = th.device("cuda", hvd.local_rank())
    print("Run experiments with world size {}".format(hvd.size()))
    if args.exp_dir and not os.path.isdir(args.exp_dir):
        os.makedirs(args.exp_dir, exist_ok=True)

    mc = config["model_config"]
    P = mc["label_size"]
    model = lstm.LSTMAM(mc["feat_dim"], P, mc["hidden_size"], mc["num_layers"], mc["dropout"], True).to(dev)
    if args.seed_model:
        if not os.path.isfile(args.seed_model):
            sys.stderr.write('ERROR: The model file %s does not exist!\n' % (args.seed_model))
            sys.exit(0)
        sd = th.load(args.seed_model, map_location="cpu")["model"]
        model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
        print("=> loaded checkpoint '{}' ".format(args.seed_model))
    elif not args.synthetic:
        sys.stderr.write('ERROR: The model file %s does not exist!\n' % (args.seed_model))
        sys.exit(0)
    optimizer = optim.SGD(model, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    hvd.broadcast_parameters(model.state_dict(), root_rank=0)
    hvd.broadcast_optimizer_state(optimizer, root_rank=0)
    optimizer = hvd.DistributedOptimizer(optimizer, named_parameters=model.named_parameters())

    dc = config["decoder_config"]
    decoder_opts = lattice.LatticeFasterDecoderOptions()
    decoder_opts.beam = dc["beam"]
    decoder_opts.lattice_beam = dc["lattice_beam"]
    decoder_opts.max_active = dc["max_active"]
    decoder_opts.determinize_lattice = False
    align_opts = dict(beam=dc.get("align_beam", 10), transition_scale=1.0, self_loop_scale=0.1, acoustic_scale=0.1)
    if args.synthetic:
        tree, trans_model = synth.alignment_model(P)
        silence_ids = synth.transition_model_arrays(P)["silence_phones"]
        asr_decoder = lattice.MappedLatticeFasterRecognizer(trans_model, synth.decoding_graph_arcs(args.graph_words, P, seed=0),
                                                            acoustic_scale=dc["acoustic_scale"], decoder_opts=decoder_opts)
        aligner = chain.MappedAligner.from_models(trans_model, tree, synth.lexicon_arcs(args.graph_words, P, seed=0), **align_opts)
        log_prior = se.log_prior_from_counts(np.ones(P))
    else:
        kaldi_model = (args.trans_model or "") + "/final.mdl"
        tree = (args.trans_model or "") + "/tree"
        L_fst = (args.lang_dir or "") + "/L.fst"
        disambig = (args.lang_dir or "") + "/phones/disambig.int"
        HCLG = (args.den_dir or "") + "/HCLG.fst"
        silence_phones = (args.den_dir or "") + "/phones/silence.csl"
        for what, path in (("HCLG", HCLG), ("silence phone", silence_phones), ("trans_model", kaldi_model), ("tree", tree),
                           ("L.fst", L_fst), ("disambig", disambig), ("prior", args.prior_path or "")):
            if not os.path.isfile(path):
                sys.stderr.write('ERROR: The %s file %s does not exist!\n' % (what, path))
                sys.exit(0)
        with open(silence_phones) as f:
            silence_ids = [int(i) for i in f.readline().strip().split(':')]
        asr_decoder = lattice.MappedLatticeFasterRecognizer.from_files(kaldi_model, HCLG, None, acoustic_scale=dc["acoustic_scale"],
                                                                       decoder_opts=decoder_opts)
        trans_model = asr_decoder.trans_model
        aligner = chain.MappedAligner.from_files(kaldi_model, tree, L_fst, None, disambig, None, **align_opts)
        log_prior = se.log_prior_from_counts(se.read_kaldi_vector(args.prior_path))
    source = data.make_source(config, P, hvd.rank(), hvd.size(), with_tids=True)
    transform = None
    if args.transform is not None and os.path.isfile(args.transform):
        transform = fbank.GlobalMeanVarianceNormalization.load(args.transform)
    fb = fbank.FbankExtractor()

    args.mwe = se.mwe_settings(config, dc["acoustic_scale"]) if args.criterion == "mwe" else None
    args.ts, teacher = None, None
    if args.criterion == "ts":
        args.ts = se.ts_settings(config, dc["acoustic_scale"])
        teacher = load_teacher(args, config, dev)
    model.train()
    for epoch in range(args.num_epochs):
        run_train_epoch(model, optimizer, log_prior.to(dev), source, fb, epoch, asr_decoder, trans_model, silence_ids, aligner,
                        args, dev, transform, teacher)
        hvd.finish()
        if hvd.rank() == 0 and args.exp_dir:
            th.save({'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'epoch': epoch},
                    args.exp_dir + '/model.se.' + str(epoch) + '.tar')
    hvd.shutdown()


def load_teacher(args, config, dev):
    """The frozen teacher of -criterion ts: model_config with the keys of `teacher_config:` on top, weights from
    -teacher_model; under -synthetic without a checkpoint, a second model initialised under a fixed seed of its own."""
    tc = dict(config["model_config"])
    tc.update(config.get("teacher_config") or {})
    if tc["label_size"] != config["model_config"]["label_size"] or tc["feat_dim"] != config["model_config"]["feat_dim"]:
        sys.stderr.write('ERROR: teacher_config must keep feat_dim and label_size of model_config!\n')
        sys.exit(0)
    if args.teacher_model:
        if not os.path.isfile(args.teacher_model):
            sys.stderr.write('ERROR: The teacher model file %s does not exist!\n' % (args.teacher_model))
            sys.exit(0)
        teacher = lstm.LSTMAM(tc["feat_dim"], tc["label_size"], tc["hidden_size"], tc["num_layers"], tc["dropout"], True)
        sd = th.load(args.teacher_model, map_location="cpu")["model"]
        teacher.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
        print("=> loaded teacher checkpoint '{}' ".format(args.teacher_model))
    elif args.synthetic:
        with th.random.fork_rng(devices=[]):
            th.manual_seed(20240917)
            teacher = lstm.LSTMAM(tc["feat_dim"], tc["label_size"], tc["hidden_size"], tc["num_layers"], tc["dropout"], True)
    else:
        sys.stderr.write('ERROR: -criterion ts needs -teacher_model!\n')
        sys.exit(0)
    teacher = teacher.to(dev).eval()
    for q in teacher.parameters():
        q.requires_grad_(False)
    return teacher


def run_train_epoch(model, optimizer, log_prior, source, fb, epoch, asr_decoder, trans_model, silence_ids, aligner, args, dev,
                    transform=None, teacher=None):
    batch_time = utils.AverageMeter('Time', ':6.3f')
    losses = utils.AverageMeter('Loss', ':.4e')
    grad_norm = utils.AverageMeter('grad_norm', ':.4e')
    n_batches = max(1, int(args.sweep_size * 3600 / (12.3 * args.batch_size)))
    progress = utils.ProgressMeter(n_batches, batch_time, losses, grad_norm, prefix="Epoch: [{}]".format(epoch))
    ce_criterion = ops.CrossEntropyLoss(ignore_index=-100, reduction='sum')
    text_rng = np.random.default_rng(1000 + hvd.rank())
    spec = args.spec.epoch(hvd.rank(), epoch) if args.spec is not None else None
    end = time.time()
    for i, batch in enumerate(data.sequence_batches(source, args.batch_size, args.sweep_size, dev, epoch=epoch)):
        if args.synthetic:     # word transcripts the utterances can hold (aux carries transition-ids there)
            texts = [synth.word_transcript(text_rng, synth.num_fbank_frames(n), args.graph_words) for n in batch["lens"]]
        else:
            texts = [np.asarray(a).reshape(-1).astype(int).tolist() for a in batch["aux"]]
        if args.criterion == "ts":
            loss, se_val, ce_loss, frames, failed = se.sequence_loss_ts(model, teacher, fb, batch, asr_decoder, log_prior, args.ts,
                                                                        args.ce_ratio, ce_criterion, transform=transform,
                                                                        spec=spec)
        elif args.criterion == "mwe":
            loss, se_val, ce_loss, frames, failed = se.sequence_loss_mwe(model, fb, batch, texts, aligner, asr_decoder, trans_model,
                                                                         log_prior, args.mwe, args.ce_ratio, ce_criterion,
                                                                         transform=transform, spec=spec)
        else:
            loss, se_val, ce_loss, frames, failed = se.sequence_loss_aligned(model, fb, batch, texts, aligner, asr_decoder,
                                                                             trans_model, log_prior, args.criterion, silence_ids,
                                                                             args.ce_ratio, ce_criterion, transform=transform,
                                                                             spec=spec)
        for j in failed:
            print("Warning: failed to align utterance {}, skip the utterance for SE loss".format(batch["utt_ids"][j]))
        optimizer.zero_grad()
        loss.backward()
        norm = optim.clip_grad_norm_(optimizer, args.max_grad_norm)
        optimizer.step()
        if i % args.print_freq == 0:
            grad_norm.update(norm.item())
            losses.update(loss.item() / float(np.sum(frames)))
            batch_time.update(time.time() - end)
            if hvd.rank() == 0:
                progress.print(i)
        end = time.time()
        if hvd.rank() == 0 and args.exp_dir and i > 0 and i % args.save_freq == 0:
            th.save({'model': model.state_dict(), 'optimizer': optimizer.state_dict()},
                    args.exp_dir + '/model.se.' + str(i) + '.tar')


if __name__ == '__main__':
    main()
