"""Runner — the reference's training / evaluation / pseudo-labelling driver (lib/standard/runner.py:17-282)
over the MI355X hot path.

Same constructor, methods and control flow as the reference; what runs underneath:

  loss         ctc.CTCLoss(blank=hp.blank_idx, zero_infinity=True)  (runner.py:35; libcfm CTC kernels)
  optimizer    optim.Adafactor(lr=hp.lr, beta1, scale_parameter, relative_step)  (runner.py:36; one
               multi-tensor HIP step; hp.scale_parameter / hp.relative_step True run on the device too)
  predict      ASRNN.predict -> cfm_ctc_greedy_decode (device argmax, torch.argmax tie rule)
  labels       generate_labels (runner.py:253-281): eval-mode forward (BatchNorm running stats, no
               dropout) -> device greedy decode with <pad>/<blank> stripped ON the device (no repeat
               collapse, the reference's Vocab.decode rule) -> only surviving ids go to the host.
               Under torch.distributed (world > 1) the batches are sharded round-robin over the ranks
               and the label lists are all-gathered back into batch order.
  beam         hp.beam_size > 0 (default 0: the paths above, unchanged): the metric and the pseudo-labels decode
               with ctc.beam_search_decode (CTC prefix beam search on the device, best hypothesis, <pad> never
               emitted, the model's output lengths) instead of the argmax; with hp.decoder_lm (set_decoder_lm)
               an n-gram LM is fused into that search (hp.lm_weight, hp.word_bonus, hp.token_beam).
  align        Runner.align: ctc.forced_align of every clip's transcript against the eval-mode forward -> per word
               (word, start frame, end frame, score), in encoder output frames (no reference counterpart).
  confidence   hp.nst_min_confidence (default None: off): generate_labels force-aligns each beam hypothesis against
               the same logits and returns None for the labels whose mean per-frame log-probability along the best
               alignment is below the threshold; MelDataset.mix_datasets leaves those clips out.
  WER          myvocab.wer (jiwer's sentence-list WER; jiwer is not in this image).  hp.device_wer (default False:
               that path, unchanged): ctc.edit_distance on the device hypothesis ids against the target ids; errors,
               reference words and the loss accumulate in device tensors read once per epoch / split, and the figure
               is the corpus WER 100 * sum(errors) / sum(words) (HParams.set_device_wer).
  confusion    Runner.test(heatmap=True): the aligned pairs of ctc.edit_distance(ops=True) as a (V + 1, V + 1) count
               matrix (row: reference word, column: hypothesis word, index V: the gap) on self.confusion[split] and
               in hp.plots_dir/confusion_<split>.json (evals.py:64 builds it with sklearn and plots it).
  MWER         hp.mwer_weight (default None: the CTC loss alone, the step unchanged; HParams.set_mwer): train minimises
               ctc + weight * mean_b(mwer_b), mwer_b = ctc.mwer_loss: the expected word errors over the beam's
               hp.mwer_nbest best hypotheses of the step's own logits (no reference counterpart).  history["loss"] stays
               the CTC loss; history["mwer"] holds the epoch's mean of the term, accumulated on the device.
  transducer   hp.transducer_weight (default None: no head, the step unchanged; HParams.set_transducer, before the model
               is built): train minimises ctc + weight * sum_b(rnnt_b) / batch_size, rnnt_b = the RNN-T loss of
               model.transducer (transducer.TransducerHead) on the encoder output (no reference counterpart).
               history["loss"] stays the CTC loss; history["rnnt"] holds the epoch's mean of the term, accumulated on
               the device.  The metric, the label pass and test keep decoding with the CTC head, unless:
  transducer   hp.transducer_decode (default False; HParams.set_transducer_decode): the metric of train and test (host
  decode       WER, device_wer, the confusion matrix) and generate_labels take their token ids from
               model.transducer.decode -- the device greedy search of the transducer head (csrc/rnnt_greedy.hip, one
               launch per batch, at most hp.transducer_max_symbols tokens per frame) on the encoder output, the
               encoder's frame counts as lengths and none for the rows that pad a short last batch -- and feed them to
               the same Vocab.decode / ctc.edit_distance code.  The loss test reports stays the CTC loss.  Needs the
               head, hp.beam_size 0 and hp.nst_min_confidence None (ValueError at the start of the pass).

Dropped (outside the hot path): tqdm colours, Evals plots (losses / WER are kept on
the Runner as .history and written to hp.plots_dir/history.json), the transformer-LM weight fusion (fuse_models).
"""
from __future__ import annotations

import json
import os
from functools import reduce
from math import ceil, isnan
from statistics import mean

import torch
import torch.nn as nn

from ...ctc import EDIT_MAX_LEN, CTCLoss, beam_search_decode, edit_distance, forced_align, greedy_decode, mwer_loss
from ...optim import Adafactor
from .myvocab import wer


def _word_lists(target_strs, predicted_strs):
    """The reference's WER preparation (runner.py:151-160): drop empty targets, split predictions into
    words ('_' for empty), pad each target with '_' to its prediction's length, flatten both."""
    predicted = [predicted_strs[i] for i in range(min(len(target_strs), len(predicted_strs))) if target_strs[i] != ""]
    target = [x for x in target_strs if x != ""]
    predicted = [x.strip().split() if len(x.strip()) > 0 else ["_"] for x in predicted]
    target = [[x] for x in target]
    target = [target[i] + ["_"] * (len(predicted[i]) - len(target[i])) for i in range(len(predicted))]
    if not predicted:
        return [], []
    return reduce(lambda a, b: a + b, target), reduce(lambda a, b: a + b, predicted)


class Runner:
    def __init__(self, model, hp, lr=None, lm=False):
        self.model = model
        self.hp = hp
        self.lm = lm
        if lr is None:
            lr = hp.lr
        self.lr = lr
        self.model.to(hp.device)
        self.loss = CTCLoss(blank=hp.blank_idx, zero_infinity=True)
        # runner.py:36 builds the optimizer with hp.lr (its `lr` argument is unused there); same here
        self.optimizer = Adafactor(model.parameters(), lr=hp.lr, beta1=hp.beta1, scale_parameter=hp.scale_parameter,
                                   relative_step=hp.relative_step)
        self.history = {"loss": [], "metric": [], "val_loss": [], "val_metric": []}
        self.confusion = {}

    def set_model(self, model):
        self.__init__(model, self.hp)

    def save_model(self, finetuning=False):
        """runner.py:48-60."""
        path = self.hp.finetuning_model_path if finetuning else (
            self.hp.standard_model_path if not self.lm else self.hp.lm_model_path)
        torch.save(self.model.state_dict(), path)

    def load_model(self, model_path):
        """runner.py:61-77: keep the checkpoint's keys that exist in the model AND contain 'conformer';
        every other entry keeps the current model's value."""
        pretrained = torch.load(model_path, map_location="cpu", weights_only=True)
        self.model.cpu()
        cur = self.model.state_dict()
        keep = {k: v for k, v in pretrained.items() if k in cur and "conformer" in k}
        keep.update({k: v for k, v in cur.items() if k not in keep})
        self.model.load_state_dict(keep)
        self.model.to(self.hp.device)

    def fuse_models(self, lm_path):
        raise NotImplementedError("the transformer-LM weight fusion (runner.py:78-101) is outside the MI355X hot "
                                  "path; for n-gram shallow fusion in the decoder see HParams.set_decoder_lm")

    # ----------------------------------------------------------------------------- train / test
    def _beam_settings(self, logits, lengths):
        """What every beam search of the Runner shares -> (fp32 logits, lengths padded / truncated to the batch, the
        decoder LM's keyword arguments)."""
        if lengths is not None:
            B = logits.shape[0]
            lengths = nn.functional.pad(lengths[:B], (0, max(0, B - lengths.shape[0])))
        kw = {}
        lm = getattr(self.hp, "decoder_lm", None)
        if lm is not None:
            kw = dict(lm=lm, lm_weight=float(self.hp.lm_weight), word_bonus=float(self.hp.word_bonus),
                      token_beam=int(self.hp.token_beam) or None)
        logits = logits.float() if logits.dtype != torch.float32 else logits
        return logits, lengths, kw

    def _beam_search(self, voc, logits, lengths):
        """The hp.beam_size search of the metric and label passes -> (fp32 logits, lengths padded / truncated to the
        batch, tokens (B, 1, T) int32, counts (B, 1))."""
        logits, lengths, kw = self._beam_settings(logits, lengths)
        toks, cnt, _ = beam_search_decode(logits, lengths, beam_size=int(self.hp.beam_size), blank=voc.blank_idx,
                                          pad=voc.pad_idx, **kw)
        return logits, lengths, toks, cnt

    def _mwer(self, voc, logits, target, target_lens, lengths):
        """hp.mwer_weight set: mean over the hp.batch_size rows of ctc.mwer_loss on the step's logits (attached), the
        search through _beam_settings with width max(hp.beam_size, hp.mwer_nbest).  Rows without a target row (and
        padded rows: no frames, one empty hypothesis) contribute 0.  Nothing is read back."""
        nbest = int(self.hp.mwer_nbest)
        logits, lengths, kw = self._beam_settings(logits, lengths)
        n = min(logits.shape[0], target.shape[0])
        T = logits.shape[1]
        loss, _, _ = mwer_loss(logits[:n], target[:n], None if lengths is None else lengths[:n], target_lens[:n],
                               nbest=nbest, beam_size=max(int(getattr(self.hp, "beam_size", 0)), nbest),
                               blank=voc.blank_idx, pad=voc.pad_idx, max_labels=min(T, 511), **kw)
        return loss.sum() / self.hp.batch_size

    def _rnnt(self, encoder, target, target_lens, lengths):
        """hp.transducer_weight set: sum over the rows of the model's transducer loss on the step's encoder output
        (attached) / hp.batch_size, over the first min(rows of the encoder output, rows of target) rows, as _mwer.
        A row's frames are the encoder's (ASRNN.decoder_lengths), and none where the step's padded length vector
        `lengths` has none (the rows that pad a short last batch): such rows, and losses that are not finite,
        contribute 0 (zero_infinity).  Nothing is read back."""
        enc, enc_lens = encoder
        n = min(enc.shape[0], target.shape[0])
        frames = torch.where(lengths[:n] > 0, enc_lens[:n], torch.zeros_like(enc_lens[:n]))
        loss = self.model.transducer(enc[:n], frames, target[:n], target_lens[:n], zero_infinity=True)
        return loss.sum() / self.hp.batch_size

    def _transducer_decode_on(self):
        """hp.transducer_decode, checked against what it needs (the start of train / test / generate_labels)."""
        if not getattr(self.hp, "transducer_decode", False):
            return False
        if not hasattr(self.model, "transducer"):
            raise ValueError("hp.transducer_decode is set but the model has no transducer head: call "
                             "HParams.set_transducer before the model is built")
        if getattr(self.hp, "beam_size", 0) > 0:
            raise ValueError("hp.transducer_decode with hp.beam_size > 0: the beam search decodes with the CTC head, "
                             "so it would be unclear which head the metric and the labels come from")
        if getattr(self.hp, "nst_min_confidence", None) is not None:
            raise ValueError("hp.transducer_decode with hp.nst_min_confidence: that confidence is the score of a CTC "
                             "alignment and says nothing about a transducer hypothesis")
        return True

    def _transducer_tokens(self, encoder, lengths=None):
        """hp.transducer_decode: (tokens (B, W) int32 padded with -1, counts (B,)) of the transducer head's greedy
        search on the step's encoder output.  A row's frames follow _rnnt's rule: the encoder's
        (ASRNN.decoder_lengths), and none where the step's length vector `lengths` (padded with zeros to the batch)
        has none.  W = min(T * max_symbols, ctc.EDIT_MAX_LEN), so that edit_distance's width limit holds at any T.
        Nothing is read back."""
        enc, enc_lens = encoder
        B, T = enc.shape[:2]
        frames = enc_lens
        if lengths is not None:
            lengths = nn.functional.pad(lengths[:B].to(enc_lens.device), (0, max(0, B - lengths.shape[0])))
            frames = torch.where(lengths > 0, enc_lens, torch.zeros_like(enc_lens))
        ms = int(getattr(self.hp, "transducer_max_symbols", 2))
        out = self.model.transducer.decode(enc, frames, max_symbols=ms, max_tokens=min(T * ms, EDIT_MAX_LEN))
        return out.tokens, out.counts

    def _beam_labels(self, voc, logits, lengths, confidence=False):
        """hp.beam_size > 0: the best prefix-beam-search hypothesis per utterance as label strings (lengths: the
        model's output lengths, padded / truncated to the batch; the kernel clamps them to [0, T]).  confidence (the
        pseudo-label pass) with hp.nst_min_confidence set: None in place of a label whose confidence is below it."""
        logits, lengths, toks, cnt = self._beam_search(voc, logits, lengths)
        labels = voc.decode(toks[:, 0], cnt[:, 0])
        thr = getattr(self.hp, "nst_min_confidence", None)
        if thr is None or not confidence:
            return labels
        conf = self._confidence(voc, logits, lengths, toks[:, 0], cnt[:, 0])
        return [None if c < thr else lab for lab, c in zip(labels, conf)]

    @staticmethod
    def _confidence(voc, logits, lengths, toks, cnt):
        """Mean per-frame log-probability of the best CTC alignment of each hypothesis (toks (B, T) int32 padded with
        -1, cnt (B,)) on the logits it was decoded from: forced_align's score / max(T_b, 1), as a list of floats."""
        B, T = logits.shape[:2]
        smax = max(int(cnt.max().item()), 1)
        frames = (torch.full((B,), T, device=logits.device, dtype=torch.int32) if lengths is None
                  else lengths.to(torch.int32).clamp(0, T))
        score = forced_align(logits, toks[:, :smax].clamp(min=0), frames, cnt, blank=voc.blank_idx).score
        return (score / frames.clamp(min=1)).tolist()

    def _metric(self, dataset, logits, target, lengths=None, encoder=None):
        if encoder is not None:     # hp.transducer_decode: the transducer head's hypothesis
            toks, cnt = self._transducer_tokens(encoder, lengths)
            tw, pw = _word_lists(dataset.vocab.decode(target), dataset.vocab.decode(toks, cnt))
            return wer(tw, pw) * 100 if tw else 0.0
        if getattr(self.hp, "beam_size", 0) > 0:
            tw, pw = _word_lists(dataset.vocab.decode(target), self._beam_labels(dataset.vocab, logits, lengths))
            return wer(tw, pw) * 100 if tw else 0.0
        predicted = self.model.predict(logits)
        t_strs = dataset.vocab.decode(target)
        p_strs = dataset.vocab.decode(predicted)
        tw, pw = _word_lists(t_strs, p_strs)
        return wer(tw, pw) * 100 if tw else 0.0

    # ----------------------------------------------------------------------------- device metric (hp.device_wer)
    def _edit_distance(self, dataset, logits, target, target_lens, lengths=None, ops=False, encoder=None):
        """ctc.edit_distance of the ids _metric decodes -- the greedy ids of every frame with <pad> / <blank> stripped
        and no repeat collapse (hp.beam_size 0), else the best beam hypothesis -- against the target ids, over the
        first min(rows of logits, rows of target) rows (the filter of _word_lists).  Nothing is read back.  The
        hypothesis rows are as wide as the logits have frames: more than 1024 frames raise (ctc.EDIT_MAX_LEN).
        encoder (hp.transducer_decode): the ids of _transducer_tokens instead."""
        voc = dataset.vocab
        if encoder is not None:
            toks, cnt = self._transducer_tokens(encoder, lengths)
        elif getattr(self.hp, "beam_size", 0) > 0:
            _, _, toks, cnt = self._beam_search(voc, logits, lengths)
            toks, cnt = toks[:, 0], cnt[:, 0]
        else:
            x = logits.float() if logits.dtype != torch.float32 else logits
            _, toks, cnt = greedy_decode(x, None, blank=voc.blank_idx, pad=voc.pad_idx, collapse=False)
        n = min(toks.shape[0], target.shape[0])
        return edit_distance(toks[:n], target[:n], cnt[:n], target_lens[:n], ops=ops)

    def _new_accumulator(self):
        """(words (2,) int64: word errors, reference words; loss () fp64: the sum of the steps' losses), on the
        device."""
        dev = self.hp.device
        return torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)

    @staticmethod
    def _accumulate(acc, ed, loss):
        """One step into the accumulators, nothing read back.  A row with an empty target contributes nothing
        (_word_lists drops it); a NaN loss counts as 100 (runner.py:166).  ed None: the loss alone."""
        words, loss_sum = acc
        loss = loss.detach().reshape(())
        loss_sum += torch.where(torch.isnan(loss), torch.full_like(loss, 100.0), loss).double()
        if ed is not None:
            counted = ed.ref_lengths > 0
            words += torch.stack([(ed.distance * counted).sum(), ed.ref_lengths.sum()])

    @staticmethod
    def _read_accumulator(acc, steps):
        """The one read of an epoch / split -> (mean loss, corpus WER %: 0.0 when there are no words)."""
        (errors, words), loss = acc[0].tolist(), acc[1].item()
        return (loss / steps if steps else float("nan")), (100.0 * errors / words if words > 0 else 0.0)

    def _confusion_add(self, conf, ed, V):
        """conf (V + 1, V + 1) int64 += the aligned pairs of ed (ops=True): row = reference word, column =
        hypothesis word, index V = the gap.  Rows with an empty target are left out, as in the metric."""
        ldp = ed.pair_ref.shape[-1]
        live = (torch.arange(ldp, device=conf.device)[None, :] < ed.n_pairs[:, None]) & (ed.ref_lengths > 0)[:, None]
        r = torch.where(ed.pair_ref < 0, V, ed.pair_ref).clamp(max=V).long()
        h = torch.where(ed.pair_hyp < 0, V, ed.pair_hyp).clamp(max=V).long()
        conf.view(-1).index_add_(0, (r * (V + 1) + h).reshape(-1), live.reshape(-1).long())

    def _write_confusion(self, dataset, dataset_type, conf):
        V = conf.shape[0] - 1
        itos = list(dataset.vocab.itos)
        labels = [itos[i] if i < len(itos) else str(i) for i in range(V)] + ["<gap>"]
        self.confusion[dataset_type] = conf.cpu()
        d = getattr(self.hp, "plots_dir", None)
        if d:
            with open(os.path.join(d, f"confusion_{dataset_type}.json"), "w") as f:
                json.dump({"labels": labels, "matrix": self.confusion[dataset_type].tolist()}, f)

    def train(self, train_set, epochs, SpecAugment=False, use_mix=False, finetuning=False):
        """runner.py:102-182."""
        dataset_type = "mix" if use_mix else "train"
        train_size = ceil(len(train_set.idxes[dataset_type]) / self.hp.batch_size)
        want_wer = getattr(self.hp, "train_wer", True)     # WER forces a host sync per step
        device_wer = bool(getattr(self.hp, "device_wer", False))
        mwer_weight = getattr(self.hp, "mwer_weight", None)     # None: the CTC loss alone (HParams.set_mwer)
        rnnt_weight = getattr(self.hp, "transducer_weight", None)     # None: no transducer term (set_transducer)
        if rnnt_weight is not None and not hasattr(self.model, "transducer"):
            raise ValueError("hp.transducer_weight is set but the model has no transducer head: call "
                             "HParams.set_transducer before the model is built")
        rnnt_decode = self._transducer_decode_on()     # the metric from the transducer head (set_transducer_decode)
        for _ in range(epochs):
            self.model.train()
            train_set.shuffle(dataset_type)
            eloss, emetric = [], []
            acc = self._new_accumulator() if device_wer else None
            if mwer_weight is not None:     # the epoch's sum of the MWER term, on the device, read once
                mwer_sum = torch.zeros((), dtype=torch.float64, device=self.hp.device)
            if rnnt_weight is not None:     # the epoch's sum of the transducer term, on the device, read once
                rnnt_sum = torch.zeros((), dtype=torch.float64, device=self.hp.device)
            for i in range(train_size):
                batch = train_set.get_batch(i, dataset_type)
                inbatch, input_lens = batch["input"]["mels"], batch["input"]["tau"]
                target, target_lens = batch["target"]["transcripts"], batch["target"]["lens"]
                self.optimizer.zero_grad()
                encoder = None
                if rnnt_weight is not None or rnnt_decode:
                    logits, output_lengths, encoder = self.model(inbatch, input_lens, SpecAugment,
                                                                 finetuning=finetuning, return_encoder=True)
                else:
                    logits, output_lengths = self.model(inbatch, input_lens, SpecAugment, finetuning=finetuning)
                output_lengths = nn.functional.pad(output_lengths, (0, self.hp.batch_size - output_lengths.shape[0]))
                output_lengths = output_lengths.clamp(max=logits.shape[1])
                loss = self.loss(logits.transpose(0, 1), target, output_lengths, target_lens)
                objective = loss
                if mwer_weight is not None:     # ctc + weight * mean_b(mwer_b); `loss` stays the CTC loss alone
                    mwer = self._mwer(train_set.vocab, logits, target, target_lens, output_lengths)
                    objective = loss + mwer_weight * mwer
                    mwer_sum += mwer.detach().double()
                if rnnt_weight is not None:     # ... + weight * sum_b(rnnt_b) / batch_size
                    rnnt = self._rnnt(encoder, target, target_lens, output_lengths)
                    objective = objective + rnnt_weight * rnnt
                    rnnt_sum += rnnt.detach().double()
                if device_wer:     # loss and word errors stay on the device: no host sync in the step
                    objective.backward()
                    self.optimizer.step()
                    with torch.no_grad():
                        ed = self._edit_distance(train_set, logits.detach(), target, target_lens, output_lengths,
                                                 encoder=encoder if rnnt_decode else None) if want_wer else None
                        self._accumulate(acc, ed, loss)
                    continue
                cur = loss.item()
                objective.backward()
                self.optimizer.step()
                eloss.append(cur)
                if want_wer:
                    emetric.append(self._metric(train_set, logits.detach(), target, output_lengths,
                                                encoder=encoder if rnnt_decode else None))
            self._check_device_errors()
            if device_wer:
                eloss, emetric = self._read_accumulator(acc, train_size)
                self.history["loss"].append(eloss)
                self.history["metric"].append(emetric if want_wer else float("nan"))
            else:
                self.history["loss"].append(mean([100 if isnan(x) else x for x in eloss]))
                self.history["metric"].append(mean(emetric) if emetric else float("nan"))
            if mwer_weight is not None:
                self.history.setdefault("mwer", []).append(mwer_sum.item() / train_size if train_size else float("nan"))
            if rnnt_weight is not None:
                self.history.setdefault("rnnt", []).append(rnnt_sum.item() / train_size if train_size else float("nan"))
            if "validation" in train_set.idxes:
                vl, vm = self.test(train_set, "validation", finetuning=finetuning)
                self.history["val_loss"].append(vl)
                self.history["val_metric"].append(vm)
        self._write_history()
        if getattr(self.hp, "base_dir", None) is not None:
            self.save_model(finetuning)

    def test(self, test_set, dataset_type="test", heatmap=False, finetuning=False):
        """runner.py:183-252 -> (mean loss, mean WER %); with hp.device_wer (mean loss, corpus WER %).  heatmap: the
        split's confusion matrix on self.confusion[dataset_type] and in hp.plots_dir (see the module docstring)."""
        rnnt_decode = self._transducer_decode_on()
        self.model.eval()
        n = ceil(len(test_set.idxes[dataset_type]) / self.hp.batch_size)
        eloss, emetric = [], []
        device_wer = bool(getattr(self.hp, "device_wer", False))
        acc = self._new_accumulator() if device_wer else None
        conf = None
        with torch.no_grad():
            for i in range(n):
                batch = test_set.get_batch(i, dataset_type)
                inbatch, input_lens = batch["input"]["mels"], batch["input"]["tau"]
                target, target_lens = batch["target"]["transcripts"], batch["target"]["lens"]
                encoder = None
                if rnnt_decode:
                    logits, output_lens, encoder = self.model(inbatch, input_lens, finetuning=finetuning,
                                                              return_encoder=True)
                else:
                    logits, output_lens = self.model(inbatch, input_lens, finetuning=finetuning)
                output_lens = nn.functional.pad(output_lens, (0, self.hp.batch_size - output_lens.shape[0]))
                output_lens = output_lens.clamp(max=logits.shape[1])
                loss = self.loss(logits.transpose(0, 1), target, output_lens, target_lens)
                if heatmap or device_wer:
                    ed = self._edit_distance(test_set, logits, target, target_lens, output_lens, ops=heatmap,
                                             encoder=encoder)
                if heatmap:
                    V = logits.shape[-1]
                    if conf is None:
                        conf = torch.zeros(V + 1, V + 1, dtype=torch.int64, device=logits.device)
                    self._confusion_add(conf, ed, V)
                if device_wer:
                    self._accumulate(acc, ed, loss)
                    continue
                eloss.append(loss.item())
                emetric.append(self._metric(test_set, logits, target, output_lens, encoder=encoder))
        self._check_device_errors()
        if conf is not None:
            self._write_confusion(test_set, dataset_type, conf)
        if device_wer:
            return self._read_accumulator(acc, n)
        eloss = mean([100 if isnan(x) else x for x in eloss])
        return eloss, mean(emetric)

    # ----------------------------------------------------------------------------- NST labels
    def generate_labels(self, dataset):
        """runner.py:253-281: pseudo-labels for every clip of dataset's 'pretrain' split, in order.  With
        hp.nst_min_confidence set, a label whose confidence (Runner._confidence) is below it is None."""
        rnnt_decode = self._transducer_decode_on()
        if getattr(self.hp, "nst_min_confidence", None) is not None and getattr(self.hp, "beam_size", 0) <= 0:
            raise ValueError("hp.nst_min_confidence needs hp.beam_size > 0: the greedy label path does not collapse "
                             "repeated frames (Vocab.decode, the reference's rule), so its labels generally have no "
                             "CTC alignment to take a confidence from")
        self.model.eval()
        n = ceil(len(dataset.idxes["pretrain"]) / self.hp.batch_size)
        voc = dataset.vocab
        world, rank = 1, 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
        mine = {}
        with torch.no_grad():
            for i in range(rank, n, world):
                batch = dataset.get_batch(i, "pretrain")["input"]
                if rnnt_decode:     # the transducer head's hypothesis, nothing from the CTC head
                    _, out_lens, encoder = self.model(batch["mels"], batch["tau"], return_encoder=True)
                    mine[i] = voc.decode(*self._transducer_tokens(encoder, out_lens))
                    continue
                logits, out_lens = self.model(batch["mels"], batch["tau"])
                if getattr(self.hp, "beam_size", 0) > 0:
                    mine[i] = self._beam_labels(voc, logits, out_lens, confidence=True)
                    continue
                # ASRNN.predict + Vocab.decode in one device pass: argmax, <pad>/<blank> removed, no collapse
                _, toks, cnt = greedy_decode(logits, None, blank=voc.blank_idx, pad=voc.pad_idx, collapse=False)
                mine[i] = voc.decode(toks, cnt)
        self._check_device_errors()
        if world > 1:
            parts = [None] * world
            torch.distributed.all_gather_object(parts, mine)
            for p in parts:
                mine.update(p)
        targets = []
        for i in range(n):
            targets += mine[i]
        return targets

    # ----------------------------------------------------------------------------- forced alignment
    def align(self, dataset, dataset_type="test"):
        """Where each word of each clip's transcript lies: an eval-mode forward per batch (as test()), then
        ctc.forced_align of the transcript against the logits.  Returns, per clip in dataset order, a list of
        (word, start_frame, end_frame, token_score) over the clip's transcript: the word's label occupies the frames
        [start_frame, end_frame) and token_score is the sum of its frames' log-probabilities.  Frames are encoder
        output frames (rows of the model's output, after the convolutional subsampling), not seconds.  A clip whose
        transcript cannot be aligned (fewer frames than labels plus repeated neighbours) gets -1, -1, 0.0 per word."""
        self.model.eval()
        n = ceil(len(dataset.idxes[dataset_type]) / self.hp.batch_size)
        voc = dataset.vocab
        out = []
        with torch.no_grad():
            for i in range(n):
                batch = dataset.get_batch(i, dataset_type)
                target, target_lens = batch["target"]["transcripts"], batch["target"]["lens"]
                logits, output_lens = self.model(batch["input"]["mels"], batch["input"]["tau"])
                output_lens = nn.functional.pad(output_lens, (0, self.hp.batch_size - output_lens.shape[0]))
                output_lens = output_lens.clamp(min=0, max=logits.shape[1])
                a = self.model.align(logits, target, output_lens, target_lens)
                ids, lens = target.tolist(), target_lens.tolist()
                starts, ends, tsc = a.starts.tolist(), a.ends.tolist(), a.token_scores.tolist()
                for b in range(batch["unpadded_len"]):
                    out.append([(voc.itos[ids[b][u]], starts[b][u], ends[b][u], tsc[b][u]) for u in range(lens[b])])
        self._check_device_errors()
        return out

    def _check_device_errors(self):
        """End-of-pass synchronising check of the BiLSTM recurrences' wait-limit flags: each forward only polls
        the flags of EARLIER passes (no host sync per launch), so a failure in the last pass of an epoch / test /
        label pass would otherwise go unreported."""
        from ...lstm import LSTM
        if any(isinstance(m, LSTM) for m in self.model.modules()):
            LSTM.check_errors()

    def _write_history(self):
        d = getattr(self.hp, "plots_dir", None)
        if d:
            with open(os.path.join(d, "history.json"), "w") as f:
                json.dump(self.history, f)
