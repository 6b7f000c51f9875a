"""HParams — the reference's hyper-parameter surface (lib/hparams.py:1-145), plus build knobs.

Same attribute names, defaults and setters as the reference so existing driver code keeps
working; the values are grouped by the subsystem that reads them.  Extra knobs for the
MI355X build (documented in DESIGN.md):

  compute_dtype          'bf16' | 'fp32'   dtype of activations / MFMA operands (fp32 = parity mode)
  frontend_proj          'utterance' | 'frame'   reference whole-utterance Linear (asrnn.py:28)
                                                  or per-subsampled-frame Linear (scalable)
  pos_enc                'none' | 'rel'    torchaudio MHSA or Transformer-XL relative positions
  use_group_norm         bool              GroupNorm(1, d) in place of BatchNorm1d in the Conformer conv module
                                           (torchaudio's use_group_norm: per-utterance statistics, no running
                                           statistics, no cross-replica reduce); default False
  specaug_ref_noop_masks bool              reproduce the reference's no-op masks (asrnn.py:141,165)
  dp_world_size          int               set by the data-parallel launcher
  beam_size              int               0: the reference's argmax decode; > 0: the Runner's metric and pseudo-label
                                           passes decode with a CTC prefix beam search of that width (set_beam_size)
  decoder_lm             lm.NGramLM | None an n-gram LM fused into that beam search (set_decoder_lm), weighted by
  lm_weight, word_bonus  float             lm_weight, plus word_bonus per emitted token; token_beam: the tokens each
  token_beam             int               entry is extended by (0: the default rule).  Not the reference's hp.lm
                                           flag, which means "train the transformer LM"
  nst_min_confidence     float | None      None: every pseudo-label is kept (the reference).  A number: the label
                                           pass force-aligns each beam hypothesis and drops the labels whose best
                                           alignment has a mean per-frame log-probability below it
                                           (set_nst_min_confidence; needs beam_size > 0)
  decoder_batched        bool              False: the reference's decoder call, one LSTM sequence over the whole
                                           batch (asrnn.py:252).  True: one sequence per utterance, bounded by the
                                           model's output lengths (set_decoder_batched); same state dict, but a
                                           model trained in one mode sees different decoder states in the other
  device_wer             bool              False: the reference's metric -- per batch, ids to the host, strings,
                                           jiwer's wer over targets padded with '_' (runner.py:151-160), the mean
                                           over the batches; one host synchronisation per step.  True
                                           (set_device_wer): the Runner takes the word errors with ctc.edit_distance
                                           on the device ids and accumulates errors, reference words and the loss in
                                           device tensors read once per epoch / split.  The figure then DIFFERS from
                                           the reference's: it is the corpus WER, 100 * sum(errors) / sum(reference
                                           words) over the epoch or split (0.0 without words), not a mean of batch
                                           figures over padded targets; the loss stays the mean of the per-step values
  mwer_weight            float | None      None: Runner.train minimises the CTC loss (the reference).  A number
  mwer_nbest             int               (set_mwer): it minimises ctc + mwer_weight * mean_b(mwer_b), mwer_b the
                                           expected word errors over the beam's mwer_nbest best hypotheses
                                           (ctc.mwer_loss; beam width max(beam_size, mwer_nbest)); history["loss"]
                                           stays the CTC loss, history["mwer"] records the term
  transducer_weight      float | None      None: no transducer head (the model and the step unchanged).  A number
  transducer_embed,      int               (set_transducer, BEFORE the model is built): ASRNN adds
  transducer_hidden,                       transducer.TransducerHead on the encoder output and Runner.train minimises
  transducer_joint                         ctc + transducer_weight * sum_b(rnnt_b) / batch_size; history["rnnt"]
                                           records the term, decoding stays with the CTC head unless:
  transducer_decode      bool              False: the Runner's metric, test and label passes decode with the CTC head.
  transducer_max_symbols int               True (set_transducer_decode): they decode with the transducer head's
                                           greedy search on the encoder output (TransducerHead.decode, one kernel
                                           launch), at most transducer_max_symbols tokens per frame; needs the head,
                                           beam_size 0 and no nst_min_confidence; test's loss stays the CTC loss
"""
from __future__ import annotations

import os
from math import inf  # noqa: F401  (the reference module exports it)

import torch

_PATHS = {  # lib/hparams.py:16-26 (relative to base_dir)
    "pretrained_model_path": ("model", "pretrained_weights.pth"),
    "standard_model_path": ("model", "standard_weights.pth"),
    "finetuning_model_path": ("model", "finetuning_weights.pth"),
    "lm_model_path": ("model", "lm_weights.pth"),
}

_OPTIMIZER = dict(beta1=0.9, beta=0.9, ngram=2, scale_parameter=False, relative_step=False, lr=2e-5,
                  pretraining_lr=3e-5)
_DATA = dict(batch_size=32, ntokens=1024, unk_tol=0.3, epochs=15, pretraining_epochs=100, hop_length=512,
             n_mels=40, read_mels=False, max_target_len=None, max_len=None, wpm=False,
             standard_train_type=["train-clean-360", "train-other-500"], librilight_subset="10h")
_FRONTEND = dict(pretraining_insize=1, pretraining_convsub_out_size=256, conv_sub_1_nodes=512, conv_sub_1_kernel=7,
                 conv_sub_1_stride=(2, 2), conv_sub_2_nodes=128, conv_sub_2_kernel=3, conv_sub_2_stride=(2, 2),
                 standard_linear_nodes=512)
_CONFORMER = dict(n_conformers=1, dropout=0.5, conformer_ff1_linear1_nodes=512, conformer_ff2_linear1_nodes=1024,
                  conformer_dropout=0.5, mhsa_num_heads=8, conformer_pointwise_conv1_nodes=1024,
                  conformer_pointwise_conv1_kernel=1, conformer_depthwise_conv_nodes=512,
                  conformer_depthwise_conv_kernel=33, conformer_depthwise_conv_stride=2,
                  conformer_pointwise_conv2_nodes=256, conformer_pointwise_conv2_kernel=1, conformer_size=1024,
                  rel_att=False, pretrained_conformer=False)
_PRETRAIN = dict(mask_probability=0.065, mask_value=0, target_context_vectors_size=320,
                 pretraining_conformer_out_size=64, pretraining_decoder_bidirectional=True,
                 pretraining_decoder_layers=1, encoded_features_out_size=128, mask_change_every_n_steps=10,
                 simplified_pretraining=True, alpha_loss=0.1, temperature_loss=0.1, distractors_K=5,
                 temperature_tau=2, do_pretraining=False, load_pretraining=False)
_DECODER = dict(standard_decoder_layers=1, standard_decoder_bidirectional=True, standard_decoder_nodes=512,
                projection_out_size=256, embedding_dim=64, extra_proj=False)
_SPECAUG = dict(warping_param_W=1, warping_ntimes=1, frequency_mask_param_F=5, frequency_mask_ntimes=2,
                time_multiplicity=2, pm=0.05, ps=0.05, time_mask_param_T=5, adaptive_multiplicity=False,
                adaptive_size=False)
_NST_LM = dict(nst=True, lm=False, train_lm=False, ft_lr=3e-6, ft_epochs=3, ft_train_epochs=1, lm_ntokens=256,
               lm_in_N=4, lm_out_N=4, input_embedding_size=320, lm_in_mhsa_num_heads=8, lm_out_mhsa_num_heads=8,
               lm_masked_out_mhsa_num_heads=8, lm_innner_input_nodes=512, lm_innner_output_nodes=512, lm_epochs=3,
               lm_max_len=20, just_nst=True)
_BUILD = dict(compute_dtype="bf16", frontend_proj="utterance", pos_enc="none", use_group_norm=False,
              specaug_ref_noop_masks=False, dp_world_size=1, layer_norm_eps=1e-5, bn_eps=1e-5, bn_momentum=0.1, beam_size=0,
              decoder_lm=None, lm_weight=0.0, word_bonus=0.0, token_beam=0, nst_min_confidence=None,
              decoder_batched=False, device_wer=False, mwer_weight=None, mwer_nbest=4, transducer_weight=None,
              transducer_embed=128, transducer_hidden=256, transducer_joint=256, transducer_decode=False,
              transducer_max_symbols=2)


class HParams:
    """Attribute bag with the reference's names (lib/hparams.py:14-145)."""

    def __init__(self, base_dir):
        self.base_dir = base_dir
        if base_dir is not None:
            self.data_dir = os.path.join(base_dir, "data")
            self.model_dir = os.path.join(base_dir, "model")
            self.plots_dir = os.path.join(base_dir, "results")
            for d in (self.model_dir, self.plots_dir):
                os.makedirs(d, exist_ok=True)
            for name, (sub, fn) in _PATHS.items():
                setattr(self, name, os.path.join(base_dir, sub, fn))
        self.device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        for group in (_OPTIMIZER, _DATA, _FRONTEND, _CONFORMER, _PRETRAIN, _DECODER, _SPECAUG, _NST_LM, _BUILD):
            for k, v in group.items():
                setattr(self, k, list(v) if isinstance(v, list) else v)
        # derived values (hparams.py: pretraining_linear_nodes, decoder_nodes, rel_pos_emb, ...)
        self.pretraining_linear_nodes = self.target_context_vectors_size
        self.decoder_nodes = (self.target_context_vectors_size // 2 if self.pretraining_decoder_bidirectional
                              else self.target_context_vectors_size)
        self.rel_pos_emb = self.rel_att
        self.output_embedding_size = self.input_embedding_size
        self.decoder_fc_nodes = self.projection_out_size

    # setters called by the dataset (speechcommands.py:39-46)
    def set_max_len(self, max_len):
        self.max_len = max_len

    def set_target_max_len(self, max_len):
        self.max_target_len = max_len

    def set_vocab_len(self, n):
        self.ntokens = n

    def set_standard_out_size(self, standard_out_size):
        self.standard_out_size = standard_out_size

    def set_input_dim(self, input_rows, input_cols):
        self.input_rows = input_rows
        self.input_cols = input_cols

    def set_space_index(self, space_idx):
        self.space_idx = space_idx

    def set_blank_index(self, blank_idx):
        self.blank_idx = blank_idx

    def set_beam_size(self, beam_size):
        self.beam_size = int(beam_size)

    def set_decoder_lm(self, lm, lm_weight=0.0, word_bonus=0.0, token_beam=0):
        """Fuse an lm.NGramLM into the beam search of the metric and pseudo-label passes (needs beam_size > 0);
        lm=None clears it."""
        self.decoder_lm = lm
        self.lm_weight, self.word_bonus, self.token_beam = float(lm_weight), float(word_bonus), int(token_beam)

    def set_nst_min_confidence(self, v):
        """Confidence filter of the noisy-student label pass: a pseudo-label is kept when score / max(T_b, 1) >= v,
        with score the log-probability of the best CTC alignment of the label (ctc.forced_align) and T_b the
        utterance's encoder frames; a dropped label is None and MelDataset.mix_datasets leaves its clip out.
        Needs beam_size > 0.  None (the default) switches the filter off."""
        self.nst_min_confidence = None if v is None else float(v)

    def set_decoder_batched(self, flag):
        """True: ASRNN runs the BiLSTM decoder per utterance (lstm.LSTM on the 3-D encoder output with the
        Conformer's frame counts as lengths) instead of as one sequence over the batch.  A model option like
        use_group_norm: the parameters are the same, the decoder states are not."""
        self.decoder_batched = bool(flag)

    def set_device_wer(self, flag):
        """True: the Runner's metric is the corpus word error rate 100 * sum(errors) / sum(reference words) of an
        epoch or split, from ctc.edit_distance on the device hypothesis ids (the greedy ids with <pad> / <blank>
        stripped, or the best beam hypothesis) against the target ids, accumulated on the device together with the
        loss: no host synchronisation per step.  Not the reference's figure (the mean over batches of a WER whose
        targets are padded with '_'), which False (the default) keeps."""
        self.device_wer = bool(flag)

    def set_mwer(self, weight, nbest=4):
        """MWER training (Prabhavalkar et al. 2018): with weight a number, Runner.train minimises
        ctc + weight * mean_b(mwer_b), mwer_b = ctc.mwer_loss of utterance b: the expected number of word errors over
        the `nbest` best hypotheses of a beam search (width max(beam_size, nbest), the decoder LM fused if one is set)
        on the step's own logits, the hypotheses weighted by their CTC likelihood.  The mean runs over the batch_size
        rows, as the CTC mean does.  history["loss"] stays the CTC loss alone; history["mwer"] records the term.
        None (the default) switches it off: the training step is then the reference's."""
        self.mwer_weight = None if weight is None else float(weight)
        self.mwer_nbest = int(nbest)
        if not 1 <= self.mwer_nbest <= 128:
            raise ValueError(f"mwer nbest must be in [1, 128], got {nbest}")

    def set_transducer(self, weight, embed=128, hidden=256, joint=256):
        """A transducer head beside the CTC head (transducer.TransducerHead on the encoder output, taken before the
        BiLSTM decoder): with weight a number, ASRNN builds the head as model.transducer and Runner.train minimises
        ctc + weight * sum_b(rnnt_b) / batch_size, rnnt_b the RNN-T loss of utterance b (transducer.rnnt_loss).
        history["loss"] stays the CTC loss alone; history["rnnt"] records the term.  The metric, the label pass and
        test keep decoding with the CTC head (set_transducer_decode switches them to this head).  A MODEL option
        like use_group_norm: set it before the model is built
        (the head adds parameters to the state dict).  None (the default): no head, the model and the step unchanged.
        embed / hidden / joint: the prediction network's embedding and LSTM widths (hidden a multiple of 8, at most
        1024: lstm.LSTM) and the joint network's width."""
        self.transducer_weight = None if weight is None else float(weight)
        self.transducer_embed, self.transducer_hidden, self.transducer_joint = int(embed), int(hidden), int(joint)
        if self.transducer_hidden % 8 or not 8 <= self.transducer_hidden <= 1024:
            raise ValueError(f"transducer hidden must be a multiple of 8 in [8, 1024], got {hidden}")
        if self.transducer_embed < 1 or self.transducer_joint < 1:
            raise ValueError("transducer embed and joint must be positive")

    def set_transducer_decode(self, flag, max_symbols=2):
        """True: the Runner's metric (train and test, host WER, device_wer and the confusion matrix) and
        generate_labels decode with the transducer head instead of the CTC head: the model is called with
        return_encoder=True and model.transducer.decode (the device greedy search, at most max_symbols tokens per
        frame, the encoder's frame counts as lengths) gives the token ids that Vocab.decode / ctc.edit_distance take.
        The loss test reports stays the CTC loss.  Needs a model built with set_transducer, beam_size 0 (it would be
        unclear which head decodes) and nst_min_confidence None (that confidence is a CTC alignment score): the
        Runner raises ValueError otherwise.  False (the default): every pass as before."""
        self.transducer_decode = bool(flag)
        self.transducer_max_symbols = int(max_symbols)
        if self.transducer_max_symbols < 1:
            raise ValueError(f"transducer max_symbols must be >= 1, got {max_symbols}")

    def set_ntokens(self, ntokens):
        self.ntokens = ntokens

    def set_max_value(self, max_value):
        self.max_value = int(max_value)
