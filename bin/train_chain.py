#!/usr/bin/env python
"""LF-MMI ("chain") training on MI355X -- command line of the reference's bin/train_chain.py
(same flags, same YAML schema, same checkpoint format chain.model.{epoch}.tar = {'model','optimizer',
'epoch'}), running on libpk2hip.so.

  python -m torch.distributed.run --nproc-per-node 8 bin/train_chain.py -config configs/mmi.yaml \
      -data configs/data.yaml -exp_dir exp/chain -chain_dir exp/chain_tree -lr 1e-3 -batch_size 4

No Kaldi here: <chain_dir>/den.fst, <chain_dir>/0.trans_mdl, <chain_dir>/tree and
<ali_dir>/final.mdl are read by the library's own readers, and the per-utterance supervision is built from the
transition-id alignment (`label`) by the library's SplitToPhones / AlignmentToProtoSupervision /
ProtoSupervisionToSupervision (pykaldi2_amd.chain, csrc/chain_sup.hip), with the reference's options
(frame_subsampling_factor 3, tolerances 5, convert_to_pdfs).  -synthetic trains on the seeded
LibriSpeech-shaped generator with a synthetic denominator graph, tree and transition model.

-e2e (no counterpart in the reference) trains alignment-free: no -ali_dir and no transition-id labels.  The label files'
`aux_label` holds each utterance's word ids (as for train_se2.py), -lang_dir supplies L.fst and phones/disambig.int, the
chain directory's tree and 0.trans_mdl build the training graphs, and the numerator is the full sum over the graph of the
transcript at the subsampled frame count (chain.graph_supervisions).  An utterance whose transcript has no
path of its length is left out of the step and counted in the progress line.  With -synthetic the transcripts are seeded
(synth.word_transcript) over the synthetic lexicon and monophone model of train_se2.py, in the same label space.

data_config `speed_perturb: [0.9, 1.0, 1.1]` / `volume_perturb: [0.125, 2.0]` (pykaldi2_amd.augment) perturb
every utterance on the device before the features are computed.  -e2e honours both: its frame counts come from the
perturbed waveform.  Without -e2e the labels are per frame of the unperturbed audio, so a speed factor other than 1 is
refused at start-up; the volume gain is honoured.  data_config `spec_augment: true` (or a mapping of its keys)
masks the features of every training minibatch in one launch; its `time_warp` moves frames, so it too needs -e2e.
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
from pykaldi2_amd import augment, beamform, chain, data, dereverb, fbank, hvd, lstm, ops, optim, synth, utils  # noqa: E402
from pykaldi2_amd.lattice import TransitionModel  # noqa: E402
from pykaldi2_amd.tree import ContextDependency  # noqa: E402


def parse_config(argv=None):
    """Command line + YAML merge of the reference script (same flags, same keys; keys this framework does not use pass through
    untouched): returns (args, config).  tests/test_host_logic.py pushes the reference's own configs/*.yaml through it."""
    parser = argparse.ArgumentParser()
    parser.add_argument("-config")
    parser.add_argument("-data", help="data yaml file")
    parser.add_argument("-dataPath", default='', type=str, help="path of data files")
    parser.add_argument("-seed_model", default='', help="the seed nerual network model")
    parser.add_argument("-exp_dir", help="the directory to save the outputs")
    parser.add_argument("-transform", help="feature transformation matrix or mvn statistics")
    parser.add_argument("-ali_dir", help="the directory to load trans_model and tree used for alignments")
    parser.add_argument("-lang_dir", help="the lexicon directory to load L.fst")
    parser.add_argument("-chain_dir", help="the directory to load trans_model, tree and den.fst for chain model")
    parser.add_argument("-lr", type=float, default=1e-3, help="set the base learning rate")
    parser.add_argument("-warmup_steps", default=4000, type=int, help="the number of warmup steps to adjust the learning rate")
    parser.add_argument("-xent_regularize", default=0, type=float, help="cross-entropy regularization weight")
    parser.add_argument("-momentum", default=0, type=float, help="set the momentum")
    parser.add_argument("-weight_decay", default=1e-4, type=float, help="set the L2 regularization weight")
    parser.add_argument("-batch_size", default=32, type=int, help="Override the batch size in the config")
    parser.add_argument("-data_loader_threads", default=0, type=int, help="number of workers for data loading")
    parser.add_argument("-max_grad_norm", default=5, type=float, help="max_grad_norm for gradient clipping")
    parser.add_argument("-sweep_size", default=100, type=float, help="process n hours of data per sweep (default:100)")
    parser.add_argument("-length_bucketed", action="store_true", help="data parallel: the ranks of one step get utterances "
                        "of similar length (a step waits at the gradient all-reduce for its longest minibatch)")
    parser.add_argument("-num_epochs", default=1, type=int, help="number of training epochs (default:1)")
    parser.add_argument("-anneal_lr_epoch", default=2, type=int, help="start to anneal the learning rate from this epoch")
    parser.add_argument("-anneal_lr_ratio", default=0.5, type=float, help="the ratio to anneal the learning rate ratio")
    parser.add_argument('-print_freq', default=10, type=int, metavar='N', help='print frequency (default: 10)')
    parser.add_argument('-save_freq', default=1000, type=int, metavar='N', help='save model frequency (default: 1000)')
    parser.add_argument('-synthetic', action='store_true', help='seeded synthetic utterances and denominator graph')
    parser.add_argument('-den_states', default=30000, type=int, help='(synthetic) denominator graph states')
    parser.add_argument('-den_arcs', default=1000000, type=int, help='(synthetic) denominator graph arcs')
    parser.add_argument('-e2e', action='store_true', help='alignment-free LF-MMI: the numerator sums over the training graph '
                        'of the word transcript (aux_label); needs -lang_dir and -chain_dir, no -ali_dir')
    parser.add_argument('-transition_scale', default=0.0, type=float, help='(-e2e) transition scale of the training graphs')
    parser.add_argument('-self_loop_scale', default=0.0, type=float, help='(-e2e) self-loop scale of the training graphs')
    parser.add_argument('-graph_words', default=200, type=int, help='(-e2e -synthetic) words of the synthetic lexicon')
    args = parser.parse_args(argv)

    with open(args.config) as f:
        config = yaml.safe_load(f)
    config["sweep_size"] = args.sweep_size
    if args.data and not args.synthetic:
        with open(args.data) as f:
            d = yaml.safe_load(f)
            config["source_paths"] = [j for i, j in d['clean_source'].items()]
            if 'dir_noise' in d:      # reference bin/train_ce.py:73-76
                config["dir_noise_paths"] = [j for i, j in d['dir_noise'].items()]
            if 'rir' in d:
                config["rir_paths"] = [j for i, j in d['rir'].items()]
    config["synthetic"] = args.synthetic
    config["data_path"] = args.dataPath
    print("pytorch version:{}".format(th.__version__))
    print("Experiment starts with config {}".format(json.dumps(config, sort_keys=True, indent=4)))
    return args, config


def main():
    args, config = parse_config()
    if not args.e2e:      # the supervision is built from frame-level labels; -e2e takes its frame count from the waveform
        augment.refuse_speed_perturb(config, "train_chain.py without -e2e")
        augment.refuse_time_warp(config, "train_chain.py without -e2e")
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
    if args.seed_model:   # weights only; a "module." prefix is stripped (reference bin/train_chain.py:147-160)
        sd = th.load(args.seed_model, map_location="cpu")["model"]
        model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
    optimizer = optim.Adam(model, lr=args.lr, amsgrad=True)
    hvd.broadcast_parameters(model.state_dict(), root_rank=0)
    hvd.broadcast_optimizer_state(optimizer, root_rank=0)
    optimizer = hvd.DistributedOptimizer(optimizer, named_parameters=model.named_parameters())

    if args.synthetic:
        den = chain.DenominatorGraph(synth.den_graph_arcs(args.den_states, args.den_arcs, P, seed=0, loop_pdf_differs=True), P)
        if args.e2e:     # monophone 3-state model and the lexicon of its word loop, pdfs in the same label space
            chain_tree, chain_trans_model = synth.alignment_model(P)
            aligner = chain.MappedAligner.from_models(chain_trans_model, chain_tree, synth.lexicon_arcs(args.graph_words, P, seed=0))
        else:
            chain_tree, chain_trans_model = synth.chain_model(P, seed=0)
            aligner = chain.MappedAligner(chain_trans_model)
    elif args.e2e:
        paths = {"chain denominator graph": os.path.join(args.chain_dir or "", "den.fst"),
                 "trans_model": os.path.join(args.chain_dir or "", "0.trans_mdl"),
                 "chain tree": os.path.join(args.chain_dir or "", "tree"),
                 "lexicon": os.path.join(args.lang_dir or "", "L.fst")}
        for what, path in paths.items():
            if not os.path.isfile(path):
                sys.stderr.write('ERROR: The {} {} does not exist!\n'.format(what, path))
                sys.exit(0)
        den = chain.DenominatorGraph(paths["chain denominator graph"], P)
        chain_trans_model = TransitionModel.read(paths["trans_model"])
        chain_tree = ContextDependency.read(paths["chain tree"])
        aligner = chain.MappedAligner.from_files(paths["trans_model"], paths["chain tree"], paths["lexicon"], None,
                                                 os.path.join(args.lang_dir or "", "phones/disambig.int"))
    else:
        den_path = os.path.join(args.chain_dir or "", "den.fst")
        chain_model_path = os.path.join(args.chain_dir or "", "0.trans_mdl")
        for what, path in (("chain denominator graph", den_path), ("trans_model", chain_model_path),
                           ("chain tree", os.path.join(args.chain_dir or "", "tree")),
                           ("alignment model", os.path.join(args.ali_dir or "", "final.mdl"))):
            if not os.path.isfile(path):     # reference bin/train_chain.py:171-177: message, exit status 0
                sys.stderr.write('ERROR: The {} {} does not exist!\n'.format(what, path))
                sys.exit(0)
        den = chain.DenominatorGraph(den_path, P)
        chain_trans_model = TransitionModel.read(chain_model_path)
        chain_tree = ContextDependency.read(os.path.join(args.chain_dir, "tree"))
        aligner = chain.MappedAligner.from_files(os.path.join(args.ali_dir, "final.mdl"), os.path.join(args.ali_dir, "tree"),
                                                 os.path.join(args.lang_dir or "", "L.fst"), None,
                                                 os.path.join(args.lang_dir or "", "phones/disambig.int"))
    supervision_opts = chain.SupervisionOptions()
    chain_opts = chain.ChainTrainingOptions(leaky_hmm_coefficient=1e-4, xent_regularize=args.xent_regularize)
    source = data.make_source(config, P, hvd.rank(), hvd.size(), ali_model=None if args.e2e else aligner.transition_model)
    transform = None
    if args.transform is not None and os.path.isfile(args.transform):
        transform = fbank.GlobalMeanVarianceNormalization.load(args.transform)
    sup_model = (aligner, chain_tree, chain_trans_model)
    fb = fbank.FbankExtractor()

    model.train()
    for epoch in range(args.num_epochs):
        run_train_epoch(model, optimizer, source, fb, epoch, supervision_opts, den, chain_opts, args, dev, sup_model, transform)
        hvd.finish()      # collective: a persistent-kernel time-out of the last steps stops every rank before the checkpoint
        if hvd.rank() == 0 and args.exp_dir:
            th.save({'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'epoch': epoch},
                    args.exp_dir + '/chain.model.' + str(epoch) + '.tar')
    hvd.shutdown()


def run_train_epoch(model, optimizer, source, fb, epoch, supervision_opts, den, chain_opts, args, dev, sup_model, transform):
    batch_time = utils.AverageMeter('Time', ':6.3f')
    losses = utils.AverageMeter('Loss', ':.4e')
    grad_norm = utils.AverageMeter('grad_norm', ':.4e')
    n_batches = max(1, int(args.sweep_size * 3600 / (12.3 * args.batch_size)))
    no_path = utils.AverageMeter('no_path', ':d')      # (-e2e) utterances left out: no path of their length
    meters = (batch_time, losses, grad_norm) + ((no_path,) if args.e2e else ())
    progress = utils.ProgressMeter(n_batches, *meters, prefix="Epoch: [{}]".format(epoch))
    sub = supervision_opts.frame_subsampling_factor
    text_rng = np.random.default_rng(4321 + epoch + hvd.rank())
    spec = args.spec.epoch(hvd.rank(), epoch) if args.spec is not None else None
    end = time.time()
    for i, batch in enumerate(data.sequence_batches(source, args.batch_size, args.sweep_size, dev, epoch=epoch,
                                                         length_bucketed=args.length_bucketed)):
        frame_shift = (epoch % sub) * -1
        feats, frames, row_off = fb(batch["wav"], batch["lens"])
        if transform is not None:     # dataset.transform of the reference (bin/train_chain.py:118-122)
            feats = transform(feats)
        if spec is not None:          # SpecAugment: masks always, the time warp under -e2e only
            feats = spec(feats, row_off, frames)
        x = fb.pad_roll_subsample(feats, row_off, frames, shift=frame_shift, subsample=sub, time_major=True)
        aligner, tree, trans_model = sup_model
        if args.e2e:
            sub_frames = [-(-int(T) // sub) for T in frames]
            if args.synthetic:
                texts = [synth.word_transcript(text_rng, T, args.graph_words) for T in sub_frames]
            else:
                texts = [np.asarray(a).reshape(-1).astype(int).tolist() for a in batch["aux"]]
            sups = chain.graph_supervisions(aligner, texts, sub_frames, args.transition_scale, args.self_loop_scale)
            skipped = [j for j, st in enumerate(sups.status) if st != chain.ALIGN_OK]
            for j in skipped:
                print("Warning: no path of {} frames for utterance {}, skip the utterance".format(sub_frames[j], batch["utt_ids"][j]))
            no_path.sum += len(skipped)
            no_path.val, no_path.avg = len(skipped), no_path.sum
        else:
            sups = [chain.supervision_from_alignment(aligner, tree, trans_model, supervision_opts, np.asarray(y)[:T])
                    for y, T in zip(batch["y"], frames)]    # reference bin/train_chain.py:262-272
        prediction = model.forward_time_major(x).transpose(0, 1)
        loss = ops.ChainObjtiveBatch.apply(prediction, den, sups, chain_opts)
        optimizer.zero_grad()
        loss.backward()
        step = n_batches * epoch + i + 1
        lr = utils.noam_decay(step, args.warmup_steps, args.lr)
        for param_group in optimizer.param_groups:
            param_group['lr'] = lr
        norm = optim.clip_grad_norm_(optimizer, args.max_grad_norm)
        optimizer.step()
        if i % args.print_freq == 0:   # .item() synchronises: only when printing
            grad_norm.update(norm.item())
            losses.update(loss.item() / float(np.sum(frames)))
            batch_time.update(time.time() - end)
            if hvd.rank() == 0:
                progress.print(i)
        end = time.time()
        if hvd.rank() == 0 and args.exp_dir and i > 0 and i % args.save_freq == 0:
            th.save({'model': model.state_dict(), 'optimizer': optimizer.state_dict()},
                    args.exp_dir + '/chain.model.' + str(i) + '.tar')


if __name__ == '__main__':
    main()
