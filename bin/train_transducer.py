#!/usr/bin/env python
"""Transducer (RNN-T) training of the LSTMAM (or, with -transformer, the TransformerAM) as the encoder of a STATELESS
transducer on whole utterances on MI355X: the phone sequence of the word transcript is the target, ops.TransducerLoss
(csrc/transducer.hip) the criterion.  No counterpart in the reference; the command line and the data path
are those of bin/train_ctc.py:

  python bin/train_transducer.py -config configs/mmi.yaml -data configs/data.yaml -exp_dir exp/td -lang_dir data/lang
  python bin/train_transducer.py -config configs/mmi.yaml -exp_dir exp/td -synthetic -batch_size 4 -sweep_size 1

The encoder has one output per phone and a blank behind them (the last column): am [N, T, V].  The predictor is a [V, V]
table of previous-label rows, lm[n, u, :] = table[prev_u] with prev_0 the blank's row and prev_u = l_u, gathered by torch
indexing; the joint is the sum am[t] + lm[u].  The table has a small Adam of its own (its gradient is all-reduced with
hvd.allreduce_), optim.Adam owns the encoder's flat buffer.  A progress line carries the loss per frame and the phone error
rate of the greedy decoding (transducer.greedy_decode); the sweep's totals are printed at its end.  Checkpoints:
exp_dir/transducer.model.{epoch}.tar = {'model', 'table', 'joiner', 'optimizer', 'table_optimizer', 'epoch'}.

With -joiner J the additive loss becomes the first of two stages (k2's pruned recipe): it also returns, per
frame, the band of -prune_range predictor rows that its occupancies favour.  Three small torch.nn.Linear layers (V -> J on the
encoder's logits, V -> J on the table rows, J -> V behind the join) make a nonlinear joiner that ops.PrunedJoin evaluates on
that band only and ops.PrunedTransducerLoss scores (csrc/transducer_pruned.hip); the loss is simple_scale * simple + pruned.
The layers are trained by the table's optimiser and their gradients all-reduced as the table's is.  The printed greedy phone
error rate is that of the ADDITIVE head.

With -beam B (and -beam_tokens K) a print step also runs transducer.beam_search (csrc/transducer_beam.hip)
and prints its phone error rate next to the greedy one: that of the additive head, and with -joiner also the joiner's,
decoded through the joiner.
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
from pykaldi2_amd import augment, beamform, data, dereverb, fbank, hvd, lstm, ops, optim, score, synth, transducer, transformer, utils  # noqa: E402


def parse_config(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-config")
    parser.add_argument("-data", help="data yaml file")
    parser.add_argument("-dataPath", default='', type=str, help="path of data files")
    parser.add_argument("-seed_model", default='', help="the seed nerual network model")
    parser.add_argument("-exp_dir", help="the directory to save the outputs")
    parser.add_argument("-transform", help="feature transformation matrix or mvn statistics")
    parser.add_argument("-lang_dir", help="the lexicon directory: phones/align_lexicon.int")
    parser.add_argument("-lr", type=float, default=1e-3, help="set the base learning rate")
    parser.add_argument("-warmup_steps", default=1000, type=int, help="the number of warmup steps to adjust the learning rate")
    parser.add_argument("-batch_size", default=32, type=int, help="Override the batch size in the config")
    parser.add_argument("-max_grad_norm", default=5, type=float, help="max_grad_norm for gradient clipping")
    parser.add_argument("-sweep_size", default=100, type=float, help="process n hours of data per sweep (default:100)")
    parser.add_argument("-num_epochs", default=1, type=int, help="number of training epochs (default:1)")
    parser.add_argument('-print_freq', default=10, type=int, metavar='N', help='print frequency (default: 10)')
    parser.add_argument("-subsample", default=3, type=int, help="frame subsampling factor in front of the network")
    parser.add_argument('-synthetic', action='store_true', help='seeded synthetic utterances, lexicon and transcripts')
    parser.add_argument('-graph_words', default=200, type=int, help='(-synthetic) words of the synthetic lexicon')
    parser.add_argument('-transformer', action='store_true', help='TransformerAM instead of LSTMAM')
    parser.add_argument("-nheads", default=4, type=int, help="(-transformer) the number of attention heads")
    parser.add_argument("-dim_model", default=512, type=int, help="(-transformer) the model dimension")
    parser.add_argument("-ff_size", default=2048, type=int, help="(-transformer) the size of feed-forward layer")
    parser.add_argument("-nlayers", default=6, type=int, help="(-transformer) the number of layers")
    parser.add_argument("-table_lr", type=float, default=1e-2, help="learning rate of the predictor table's optimiser")
    parser.add_argument("-max_symbols", default=8, type=int, help="phones the greedy decoding may emit per frame")
    parser.add_argument("-joiner", default=0, type=int, metavar='J', help="train a nonlinear joiner of width J on the pruned band "
                        "(the second stage); the greedy error rate stays the additive head's, -beam also decodes through the joiner")
    parser.add_argument("-prune_range", default=5, type=int, metavar='S', help="(-joiner) predictor rows per frame in the band")
    parser.add_argument("-simple_scale", default=0.5, type=float, metavar='X', help="(-joiner) the loss is X * simple + pruned")
    parser.add_argument("-beam", default=0, type=int, metavar='B', help="also decode the printed minibatches by beam search of width B "
                        "(at most min(max_symbols, 31) phones per frame) and print its phone error rate")
    parser.add_argument("-beam_tokens", default=8, type=int, metavar='K', help="(-beam) phones that may extend a hypothesis per round")
    args = parser.parse_args(argv)
    with open(args.config) as f:
        config = yaml.safe_load(f)
    config["sweep_size"] = args.sweep_size
    if args.data and not args.synthetic:
        with open(args.data) as f:
            d = yaml.safe_load(f)
            config["source_paths"] = [j for i, j in d['clean_source'].items()]
            if 'dir_noise' in d:
                config["dir_noise_paths"] = [j for i, j in d['dir_noise'].items()]
            if 'rir' in d:
                config["rir_paths"] = [j for i, j in d['rir'].items()]
    config["synthetic"] = args.synthetic
    config["data_path"] = args.dataPath
    print("Experiment starts with config {}".format(json.dumps(config, sort_keys=True, indent=4)))
    return args, config


def first_pronunciations(args, num_pdfs):
    """{word id: [phone ids, 1-based]} of each word's first pronunciation, and the number of phones."""
    prons = {}
    if args.synthetic:      # the word loop of synth.lexicon_arcs: a word starts on the arc that carries its id
        lex = synth.lexicon_arcs(args.graph_words, num_pdfs, seed=0)
        word = 0
        for ph, w in zip(lex["ilabel"].tolist(), lex["olabel"].tolist()):
            word = w or word
            prons.setdefault(word, []).append(ph)
        return prons, num_pdfs // 3
    path = os.path.join(args.lang_dir or "", "phones", "align_lexicon.int")
    if not os.path.isfile(path):
        sys.stderr.write('ERROR: The lexicon {} does not exist!\n'.format(path))
        sys.exit(0)
    with open(path) as f:
        for line in f:
            p = [int(tok) for tok in line.split()]
            if len(p) >= 3:
                prons.setdefault(p[0], p[2:])
    return prons, max(max(p) for p in prons.values())


def main():
    args, config = parse_config()
    args.spec = augment.SpecAugment.from_config(config)      # None without data_config spec_augment
    beamform.require_beamform_config(config, os.path.basename(sys.argv[0]))
    dereverb.require_wpe_config(config, os.path.basename(sys.argv[0]))
    hvd.init()
    th.cuda.set_device(hvd.local_rank())
    dev = th.device("cuda", hvd.local_rank())
    if args.exp_dir and not os.path.isdir(args.exp_dir):
        os.makedirs(args.exp_dir, exist_ok=True)
    mc = config["model_config"]
    args.prons, num_phones = first_pronunciations(args, mc["label_size"])
    args.blank = num_phones                                   # phone p is column p - 1, the blank the last column
    if args.transformer:
        model = transformer.TransformerAM(mc["feat_dim"], args.dim_model, args.nheads, args.ff_size, args.nlayers, mc["dropout"],
                                          num_phones + 1).to(dev)
    else:
        model = lstm.LSTMAM(mc["feat_dim"], num_phones + 1, mc["hidden_size"], mc["num_layers"], mc["dropout"], True).to(dev)
    if args.seed_model:
        sd = th.load(args.seed_model, map_location="cpu")["model"]
        model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
    table = th.zeros(num_phones + 1, num_phones + 1, device=dev, requires_grad=True)      # the predictor: row = previous label
    if args.seed_model and "table" in th.load(args.seed_model, map_location="cpu"):
        table.data.copy_(th.load(args.seed_model, map_location="cpu")["table"])
    joiner = None
    if args.joiner:      # (made only on request: a seeded run without it draws the same random numbers as before)
        joiner = th.nn.ModuleDict({"enc": th.nn.Linear(num_phones + 1, args.joiner), "pred": th.nn.Linear(num_phones + 1, args.joiner),
                                   "out": th.nn.Linear(args.joiner, num_phones + 1)}).to(dev)
        if args.seed_model and th.load(args.seed_model, map_location="cpu").get("joiner"):
            joiner.load_state_dict(th.load(args.seed_model, map_location="cpu")["joiner"])
        hvd.broadcast_parameters(joiner.state_dict(), root_rank=0)
    table_optimizer = th.optim.Adam([table] + (list(joiner.parameters()) if joiner else []), lr=args.table_lr)
    optimizer = optim.Adam(model, lr=args.lr, amsgrad=True)
    hvd.broadcast_parameters({"table": table.data}, root_rank=0)
    hvd.broadcast_parameters(model.state_dict(), root_rank=0)
    hvd.broadcast_optimizer_state(optimizer, root_rank=0)
    optimizer = hvd.DistributedOptimizer(optimizer, named_parameters=model.named_parameters())
    source = data.make_source(config, mc["label_size"], hvd.rank(), hvd.size(), ali_model=None)
    transform = None
    if args.transform is not None and os.path.isfile(args.transform):
        transform = fbank.GlobalMeanVarianceNormalization.load(args.transform)
    criterion = ops.TransducerLoss(blank=args.blank, reduction="sum", time_major=not args.transformer,
                                   prune_range=args.prune_range if joiner else None)
    args.pruned = ops.PrunedTransducerLoss(blank=args.blank, reduction="sum")
    fb = fbank.FbankExtractor()
    model.train()
    for epoch in range(args.num_epochs):
        run_train_epoch(model, table, joiner, optimizer, table_optimizer, criterion, source, fb, epoch, args, dev, transform)
        hvd.finish()
        if hvd.rank() == 0 and args.exp_dir:
            th.save({'model': model.state_dict(), 'table': table.detach().cpu(), 'optimizer': optimizer.state_dict(),
                     'joiner': joiner.state_dict() if joiner else None,
                     'table_optimizer': table_optimizer.state_dict(), 'epoch': epoch},
                    args.exp_dir + '/transducer.model.' + str(epoch) + '.tar')
    hvd.shutdown()


def run_train_epoch(model, table, joiner, optimizer, table_optimizer, criterion, source, fb, epoch, args, dev, transform):
    batch_time = utils.AverageMeter('Time', ':6.3f')
    losses = utils.AverageMeter('Loss', ':.4e')
    per = utils.AverageMeter('PER', ':.4f')
    grad_norm = utils.AverageMeter('grad_norm', ':.4e')
    beam_per = {k: utils.AverageMeter(k, ':.4f') for k in (['beamPER'] + (['joinerPER'] if joiner else []) if args.beam else [])}
    n_batches = max(1, int(args.sweep_size * 3600 / (12.3 * args.batch_size)))
    progress = utils.ProgressMeter(n_batches, batch_time, losses, per, *beam_per.values(), grad_norm, prefix="Epoch: [{}]".format(epoch))
    text_rng = np.random.default_rng(4321 + epoch + hvd.rank())
    spec = args.spec.epoch(hvd.rank(), epoch) if args.spec is not None else None
    sub = args.subsample
    end = time.time()
    for i, batch in enumerate(data.sequence_batches(source, args.batch_size, args.sweep_size, dev, epoch=epoch)):
        feats, frames, row_off = fb(batch["wav"], batch["lens"])
        if transform is not None:
            feats = transform(feats)
        if spec is not None:
            feats = spec(feats, row_off, frames)
        x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=sub, time_major=True)
        sub_frames = [-(-int(T) // sub) for T in frames]
        if args.synthetic:
            texts = [synth.word_transcript(text_rng, T, args.graph_words) for T in sub_frames]
        else:
            texts = [np.asarray(a).reshape(-1).astype(int).tolist() for a in batch["aux"]]
        labels = [[ph - 1 for w in text for ph in args.prons[w]] for text in texts]
        if args.transformer:
            prediction = transformer.padded_forward(model, x, sub_frames)      # [N, Tmax, P]
        else:
            prediction = model.forward_time_major(x)                           # [Tmax, N, P]
        umax = max(len(lab) for lab in labels)
        prev = th.tensor([[args.blank] + lab + [args.blank] * (umax - len(lab)) for lab in labels], device=dev)
        lm = table[prev]                                                   # [N, umax + 1, V]
        if joiner is None:
            loss = criterion(prediction, lm, sub_frames, labels)
        else:      # the additive loss picks the band, the joiner is evaluated and scored on it
            simple, begin = criterion(prediction, lm, sub_frames, labels)
            am = prediction if args.transformer else prediction.transpose(0, 1)      # [N, Tmax, V]
            h = ops.PrunedJoin.apply(joiner["enc"](am), joiner["pred"](lm), begin, sub_frames, [len(lab) for lab in labels],
                                     args.prune_range)
            loss = args.simple_scale * simple + args.pruned(joiner["out"](h), begin, sub_frames, labels)
        optimizer.zero_grad()
        table_optimizer.zero_grad()
        loss.backward()
        hvd.allreduce_(table.grad)
        for q in (joiner.parameters() if joiner else ()):
            hvd.allreduce_(q.grad)
        table_optimizer.step()
        step = n_batches * epoch + i + 1
        lr = utils.noam_decay(step, args.warmup_steps, args.lr)
        for param_group in optimizer.param_groups:
            param_group['lr'] = lr
        norm = optim.clip_grad_norm_(optimizer, args.max_grad_norm)
        optimizer.step()
        if i % args.print_freq == 0:   # .item() and the decoding synchronise: only when printing
            hyps = transducer.greedy_decode(prediction, sub_frames, table, args.blank, args.max_symbols, time_major=not args.transformer)
            errs, words = score.wer(hyps, labels, device="cpu")
            grad_norm.update(norm.item())
            losses.update(loss.item() / float(np.sum(sub_frames)), int(np.sum(sub_frames)))
            per.update(errs / max(words, 1), words)
            if args.beam:
                kw = dict(blank=args.blank, beam=args.beam, top_tokens=args.beam_tokens, max_symbols=min(args.max_symbols, transducer.MAX_BEAM_SYMBOLS))
                found = {'beamPER': transducer.beam_search(prediction, sub_frames, table, time_major=not args.transformer, **kw)}
                if joiner:
                    with th.no_grad():
                        found['joinerPER'] = transducer.beam_search(joiner["enc"](prediction), sub_frames, joiner["pred"](table),
                                                                    joiner=(joiner["out"].weight, joiner["out"].bias),
                                                                    time_major=not args.transformer, **kw)
                for k, nbest in found.items():
                    errs, words = score.wer([h[0][0] if h else [] for h in nbest], labels, device="cpu")
                    beam_per[k].update(errs / max(words, 1), words)
            batch_time.update(time.time() - end)
            if hvd.rank() == 0:
                progress.print(i)
        end = time.time()
    if hvd.rank() == 0:
        print("Epoch {}: loss per frame {:.4f}, greedy phone error rate {:.4f} (over the printed minibatches)".format(
            epoch, losses.avg, per.avg))
        for k, m in beam_per.items():
            print("Epoch {}: beam {} phone error rate {:.4f} ({})".format(epoch, args.beam, m.avg, k))


if __name__ == '__main__':
    main()
