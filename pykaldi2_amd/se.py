"""One sequence-discriminative training step (lattice MMI / sMBR / MPFE + CE regulariser) for a whole
minibatch on the device: the body of the reference's bin/train_se.py:226-262 without its per-utterance Python
loop and host round trips.

    prediction = model(x)                                           bin/train_se.py:231
    ce_loss = CrossEntropyLoss(ignore_index=-100, reduction='sum')  :214,235
    se_loss = sum_j criterion(prediction[j, :num_frs[j]] - log_prior, asr_decoder, trans_model, trans_id_j)  :237-249
    loss = se_loss + ce_ratio * ce_loss                             :251
"""
import numpy as np
import torch

from . import ops


def read_kaldi_vector(path):
    """Kaldi vector / single-row matrix in text (" [ 1 2 3 ]") or binary ("\\0B" + FV/DV/FM/DM) form -- the
    `final.occs` priors file (reference bin/train_se.py:186-187: read_matrix(prior_path)[0])."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\0B":
        tag = raw[2:5]
        pos = 5
        dt = np.dtype("<f4") if tag[:1] == b"F" else np.dtype("<f8")

        def rd_int(p):
            assert raw[p] == 4
            return int(np.frombuffer(raw, "<i4", 1, p + 1)[0]), p + 5
        if tag in (b"FV ", b"DV "):
            n, pos = rd_int(pos)
            return np.frombuffer(raw, dt, n, pos).astype(np.float64)
        if tag in (b"FM ", b"DM "):
            r, pos = rd_int(pos)
            c, pos = rd_int(pos)
            return np.frombuffer(raw, dt, r * c, pos).astype(np.float64).reshape(r, c)[0]
        raise ValueError("%s: unsupported Kaldi object %r" % (path, tag))
    toks = raw.decode().replace("[", " ").replace("]", " ").split()
    return np.asarray([float(t) for t in toks], np.float64)


def log_prior_from_counts(counts):
    """log(prior / sum(prior)) as float32 (reference bin/train_se.py:187)."""
    c = np.asarray(counts, np.float64)
    return torch.tensor(np.log(c / c.sum()), dtype=torch.float32)


def sequence_loss(model, fb, batch, asr_decoder, trans_model, log_prior, criterion, silence_ids, ce_ratio, ce_criterion,
                  forward=None, transform=None, spec=None):
    """Forward of one minibatch: batch = dict(wav, lens, y = pdf alignments, aux = transition-id alignments)
    from pykaldi2_amd.data.  `forward(model, x[Tmax, N, 80], frames) -> [N, Tmax, P]` replaces the BLSTM call
    (TransformerAM with its masks: bin/train_transformer_se.py).  Returns (loss, se_value, ce_loss, frames)."""
    feats, frames, row_off = fb(batch["wav"], batch["lens"])
    if transform is not None:      # the `-transform` MVN statistics (reference bin/train_se.py:104-108)
        feats = transform(feats)
    if spec is not None:
        feats = spec(feats, row_off, frames)
    x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=1, time_major=True)      # [Tmax, N, 80]
    if forward is not None:
        prediction = forward(model, x, frames)
    else:
        prediction = model.forward_time_major(x).transpose(0, 1)                                   # [N, Tmax, P] view
    N, Tmax = prediction.shape[0], prediction.shape[1]
    y = np.full((N, Tmax), -100, np.int64)
    for n, lab in enumerate(batch["y"]):
        y[n, :frames[n]] = np.asarray(lab)[:frames[n]]
    ce_loss = ce_criterion(prediction, torch.from_numpy(y).to(prediction.device))
    loglikes = prediction - log_prior
    se = ops.LatticeBatchFunction.apply(loglikes, [int(t) for t in frames], asr_decoder, trans_model, batch["aux"],
                                        criterion, silence_ids)
    return se + ce_ratio * ce_loss, se, ce_loss, frames


def sequence_loss_aligned(model, fb, batch, texts, aligner, asr_decoder, trans_model, log_prior, criterion, silence_ids,
                          ce_ratio, ce_criterion, forward=None, transform=None, spec=None):
    """The step of the reference's bin/train_se2.py:240-273: the numerator alignment of every utterance is made on the fly
    from its word transcript (`texts`) with the current model -- one MappedAligner.align_batch on prediction - log_prior
    for the whole minibatch -- instead of being read from the label files.  Utterances that fail to align are left out of
    the sequence term.  loss = ce_ratio * ce_loss + sum of the sequence criterion.  Returns (loss, se_value, ce_loss,
    frames, indices of the utterances that failed)."""
    feats, frames, row_off = fb(batch["wav"], batch["lens"])
    if transform is not None:
        feats = transform(feats)
    if spec is not None:
        feats = spec(feats, row_off, frames)
    x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=1, time_major=True)
    prediction = forward(model, x, frames) if forward is not None else model.forward_time_major(x).transpose(0, 1)
    N, Tmax = prediction.shape[0], prediction.shape[1]
    y = np.full((N, Tmax), -100, np.int64)
    for n, lab in enumerate(batch["y"]):
        y[n, :frames[n]] = np.asarray(lab)[:frames[n]]
    ce_loss = ce_criterion(prediction, torch.from_numpy(y).to(prediction.device))
    loglikes = prediction - log_prior
    lengths = [int(t) for t in frames]
    ali = aligner.align_batch(loglikes.detach(), lengths, texts)
    keep = [n for n, r in enumerate(ali) if r is not None]
    failed = [n for n, r in enumerate(ali) if r is None]
    if keep:
        sub = loglikes if len(keep) == N else loglikes[keep]
        lens = [lengths[n] for n in keep]
        sub = sub[:, :max(lens)]
        se = ops.LatticeBatchFunction.apply(sub, lens, asr_decoder, trans_model, [ali[n]["alignment"] for n in keep],
                                            criterion, silence_ids)
    else:
        se = torch.zeros((), dtype=torch.float32, device=prediction.device)
    return ce_ratio * ce_loss + se, se, ce_loss, frames, failed


def mwe_settings(config, acoustic_scale):
    """The `mwe_config:` block of the YAML over its defaults (num_paths 16, lm_weight 1.0, am_weight = the decoder's
    acoustic scale, equal_weight / phone_level / rand_path / distinct false), validated as MWEFunction does."""
    from .lattice import mwe_config
    cfg = dict(num_paths=16, lm_weight=1.0, am_weight=float(acoustic_scale), equal_weight=False, phone_level=False,
               rand_path=False, distinct=False)
    cfg.update(config.get("mwe_config") or {})
    mwe_config(cfg)
    return cfg


def sequence_loss_mwe(model, fb, batch, texts, aligner, asr_decoder, trans_model, log_prior, mwe_cfg, ce_ratio, ce_criterion,
                      forward=None, transform=None, spec=None):
    """The train_se2 step with the N-best minimum word error criterion (ops.MWEBatchFunction): the supervision is the word
    transcript (`texts`); with mwe_cfg['phone_level'] it is the transition-id alignment made on the fly as in
    sequence_loss_aligned (utterances that fail to align are left out).  loss = ce_ratio * ce_loss + sum of the MWE losses.
    Returns (loss, se_value, ce_loss, frames, indices of the utterances that failed)."""
    feats, frames, row_off = fb(batch["wav"], batch["lens"])
    if transform is not None:
        feats = transform(feats)
    if spec is not None:
        feats = spec(feats, row_off, frames)
    x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=1, time_major=True)
    prediction = forward(model, x, frames) if forward is not None else model.forward_time_major(x).transpose(0, 1)
    N, Tmax = prediction.shape[0], prediction.shape[1]
    y = np.full((N, Tmax), -100, np.int64)
    for n, lab in enumerate(batch["y"]):
        y[n, :frames[n]] = np.asarray(lab)[:frames[n]]
    ce_loss = ce_criterion(prediction, torch.from_numpy(y).to(prediction.device))
    loglikes = prediction - log_prior
    lengths = [int(t) for t in frames]
    failed, keep, sups = [], list(range(N)), list(texts)
    if mwe_cfg["phone_level"]:
        ali = aligner.align_batch(loglikes.detach(), lengths, texts)
        keep = [n for n, r in enumerate(ali) if r is not None]
        failed = [n for n, r in enumerate(ali) if r is None]
        sups = [ali[n]["alignment"] if ali[n] is not None else None for n in range(N)]
    if keep:
        sub = loglikes if len(keep) == N else loglikes[keep]
        lens = [lengths[n] for n in keep]
        sub = sub[:, :max(lens)]
        se = ops.MWEBatchFunction.apply(sub, lens, asr_decoder, trans_model, [sups[n] for n in keep], mwe_cfg)
    else:
        se = torch.zeros((), dtype=torch.float32, device=prediction.device)
    return ce_ratio * ce_loss + se, se, ce_loss, frames, failed


TS_KEYS = ("lm_weight", "am_weight", "old_acoustic_scale")


def ts_settings(config, acoustic_scale):
    """The `ts_config:` block of the YAML over its defaults (lm_weight 1.0, am_weight = the decoder's acoustic scale,
    old_acoustic_scale 0.0); a key it does not know raises KeyError."""
    cfg = dict(lm_weight=1.0, am_weight=float(acoustic_scale), old_acoustic_scale=0.0)
    for k, v in (config.get("ts_config") or {}).items():
        if k not in TS_KEYS:
            raise KeyError("ts_config: unknown key %r (known: %s)" % (k, ", ".join(TS_KEYS)))
        cfg[k] = float(v)
    return cfg


def sequence_loss_ts(model, teacher, fb, batch, asr_decoder, log_prior, ts_cfg, ce_ratio, ce_criterion, forward=None,
                     transform=None, spec=None):
    """The train_se2 step with the lattice teacher-student criterion (ops.TeacherStudentBatch): the frozen `teacher` runs
    under torch.no_grad() in eval mode on the same features, the lattices are decoded from its log-likelihoods and rescored
    with the student's; the log prior is subtracted from both, as the reference's docstring asks (ops/ops.py:81).
    `spec` (feats, row_off, frames, out=) augments the student's features only, out of place.
    loss = ce_ratio * ce_loss + sum of the per-utterance divergences.  Returns (loss, ts_value, ce_loss, frames, [])."""
    feats, frames, row_off = fb(batch["wav"], batch["lens"])
    if transform is not None:
        feats = transform(feats)
    x = fb.pad_roll_subsample(feats, row_off, frames, shift=0, subsample=1, time_major=True)
    x_T = x          # the teacher decodes its lattices from the clean features; only the student sees the augmented ones
    if spec is not None:
        x = fb.pad_roll_subsample(spec(feats, row_off, frames, out=torch.empty_like(feats)), row_off, frames, shift=0,
                                  subsample=1, time_major=True)
    run = (lambda m, x: forward(m, x, frames)) if forward is not None else (lambda m, x: m.forward_time_major(x).transpose(0, 1))
    was_training = teacher.training
    teacher.eval()
    with torch.no_grad():
        prediction_T = run(teacher, x_T)
    teacher.train(was_training)
    prediction = run(model, x)
    N, Tmax = prediction.shape[0], prediction.shape[1]
    y = np.full((N, Tmax), -100, np.int64)
    for n, lab in enumerate(batch["y"]):
        y[n, :frames[n]] = np.asarray(lab)[:frames[n]]
    ce_loss = ce_criterion(prediction, torch.from_numpy(y).to(prediction.device))
    ts = ops.TeacherStudentBatch.apply(prediction_T - log_prior, prediction - log_prior, [int(t) for t in frames], asr_decoder,
                                       ts_cfg["lm_weight"], ts_cfg["am_weight"], ts_cfg["old_acoustic_scale"])
    return ce_ratio * ce_loss + ts, ts, ce_loss, frames, []
