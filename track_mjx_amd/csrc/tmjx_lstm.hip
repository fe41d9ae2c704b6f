// csrc/tmjx_lstm.hip — fifth translation unit of libtmjx_hip.so: the LSTM decoder's recurrence (csrc/lstm_kernels.h) and its C-ABI entry points
// (include/tmjx.h "LSTM decoder recurrence").  Compiled next to the other units (track_mjx_amd/hip.py:build) and linked into the same library.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "lstm_kernels.h"
#include "lstm_decoder_act.h"

static bool hidden_ok(int H) { return H == 32 || H == 64 || H == 128 || H == 256; }

static const char *fwd_why(const tmjx_lstm_fwd_t *a) {
  if (!a) return "null argument block";
  if (!hidden_ok(a->H)) return "H must be 32, 64, 128 or 256";
  if (a->T < 1 || a->rows < 1) return "T >= 1 and rows >= 1";
  if (!a->xg || !a->Wh || !a->bh || !a->h0 || !a->c0 || !a->h || !a->c) return "null xg / Wh / bh / h0 / c0 / h / c";
  if (a->ldx < 4 * a->H || a->ldw < a->H || a->ld0 < a->H || a->ldo < a->H) return "ldx >= 4H, ldw >= H, ld0 >= H, ldo >= H";
  if ((a->ldw & 3) || !al16(a->Wh)) return "W_h rows must be 16-byte aligned (ldw % 4 == 0)";
  if (a->reset && a->ldr < a->rows) return "ldr >= rows";
  for (const void *p : {(const void *)a->xg, (const void *)a->bh, (const void *)a->h0, (const void *)a->c0, (const void *)a->reset, (const void *)a->h,
                        (const void *)a->c, (const void *)a->gates, (const void *)a->h_prev})
    if (!al4(p)) return "misaligned float pointer";
  if (a->T > 1 && (a->h == a->h0 || a->c == a->c0)) return "h / c may alias h0 / c0 only when T == 1";
  return nullptr;
}

static const char *bwd_why(const tmjx_lstm_bwd_t *a) {
  if (!a) return "null argument block";
  if (!hidden_ok(a->H)) return "H must be 32, 64, 128 or 256";
  if (a->T < 1 || a->rows < 1) return "T >= 1 and rows >= 1";
  if (!a->dh || !a->Wh || !a->gates || !a->c || !a->c0 || !a->dgates) return "null dh / Wh / gates / c / c0 / dgates";
  if (a->ldd < a->H || a->ldw < a->H || a->ldo < a->H || a->ld0 < a->H) return "ldd >= H, ldw >= H, ldo >= H, ld0 >= H";
  if (a->reset && a->ldr < a->rows) return "ldr >= rows";
  for (const void *p : {(const void *)a->dh, (const void *)a->Wh, (const void *)a->gates, (const void *)a->c, (const void *)a->c0, (const void *)a->reset,
                        (const void *)a->dgates, (const void *)a->dh0, (const void *)a->dc0})
    if (!al4(p)) return "misaligned float pointer";
  return nullptr;
}

static_assert(sizeof(tmjx_lstm_decoder_act_t) == 296, "tmjx_lstm_decoder_act_t: the layout hip.LstmDecoderAct declares");
static const char *decoder_act_why(const tmjx_lstm_decoder_act_t *a) {
  if (!a) return "null argument block";
  if (!a->latents || !a->obs || !a->action_t || !a->Wp) return "null argument (latents / obs / action_t / Wp)";
  if (!a->h || !a->c) return "null carry (h / c)";
  if (a->H != LDA_H) return "H must be 128";
  if (a->L < 1 || a->L > TMJX_LSTM_DECODER_MAX_LAYERS) return "1 .. 4 LSTM layers";
  if (const char *why = decoder_io_why(a)) return why;
  if (!al4(a->reset) || !al4(a->h) || !al4(a->c) || !al4(a->bp)) return "float pointers must be 4-byte aligned";
  const long long K1 = (long long)a->Z + a->obs_w - a->ref_w;
  for (int k = 0; k < a->L; k++) {
    const tmjx_lstm_decoder_layer_t &y = a->layer[k];
    if (!y.Wi || !y.Wh || !y.bh) return "null layer argument (Wi / Wh / bh)";
    if ((y.ldwi & 3) || (y.ldwh & 3) || !al16(y.Wi) || !al16(y.Wh)) return "weight rows must be 16-byte aligned (ldw % 4 == 0)";
    const long long K = k == 0 ? K1 : a->H;
    if (y.ldwi < ((K + 3) & ~3ll) || y.ldwh < a->H) return "ldwi >= the layer's input width rounded up to 4, ldwh >= H";
    if (!al4(y.bh)) return "float pointers must be 4-byte aligned";
  }
  if ((a->ldwp & 3) || !al16(a->Wp)) return "weight rows must be 16-byte aligned (ldw % 4 == 0)";
  if (a->ldwp < a->H) return "ldwp >= H";
  if (a->ld < a->L * a->H) return "the carry's ld >= L * H";
  return nullptr;
}

template <int H>
static int launch_fwd(const LstmFwd &P, hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_fwd<H>, dim3((P.rows + LSTM_RB - 1) / LSTM_RB), dim3(LSTM_NT), 0, s, P);
  return check_launch("k_lstm_fwd");
}
template <int H>
static int launch_bwd(const LstmBwd &P, hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_bwd<H>, dim3((P.rows + LSTM_RB - 1) / LSTM_RB), dim3(LSTM_NT), 0, s, P);
  return check_launch("k_lstm_bwd");
}

extern "C" {
int tmjx_lstm_hidden_ok(int H) { return hidden_ok(H); }

int tmjx_lstm_seq_fwd(const tmjx_lstm_fwd_t *a, void *stream) {
  if (const char *why = fwd_why(a)) return fail(TMJX_EINVAL, std::string("tmjx_lstm_seq_fwd: ") + why);
  const LstmFwd P{a->xg, a->ldx, a->Wh, a->ldw, a->bh, a->h0, a->c0, a->ld0, a->reset, a->ldr, a->h, a->c, a->ldo, a->gates, a->h_prev, a->T, a->rows};
  hipStream_t s = (hipStream_t)stream;
  switch (a->H) {
    case 32: return launch_fwd<32>(P, s);
    case 64: return launch_fwd<64>(P, s);
    case 128: return launch_fwd<128>(P, s);
    default: return launch_fwd<256>(P, s);
  }
}

int tmjx_lstm_decoder_act_ok(const tmjx_lstm_decoder_act_t *a) { return decoder_act_why(a) == nullptr; }
int tmjx_lstm_decoder_act(const tmjx_lstm_decoder_act_t *a, void *stream) {
  if (const char *why = decoder_act_why(a)) return fail(TMJX_EINVAL, std::string("tmjx_lstm_decoder_act: ") + why);
  LstmDecAct P{};
  P.in = decoder_in(a); P.reset = a->reset; P.L = a->L;
  for (int k = 0; k < a->L; k++) P.l[k] = LstmDecLayer{a->layer[k].Wi, a->layer[k].Wh, a->layer[k].bh, a->layer[k].ldwi, a->layer[k].ldwh};
  P.Wp = a->Wp; P.bp = a->bp; P.ldwp = a->ldwp;
  P.h = a->h; P.c = a->c; P.ld = a->ld; P.out = decoder_out(a);
  return launch_lds<k_lstm_decoder_act>("k_lstm_decoder_act", dim3((P.in.M + LDA_BM - 1) / LDA_BM), dim3(LDA_NT), sizeof(float) * (size_t)LDA_LDS_FLOATS, (hipStream_t)stream, P);
}

int tmjx_lstm_seq_bwd(const tmjx_lstm_bwd_t *a, void *stream) {
  if (const char *why = bwd_why(a)) return fail(TMJX_EINVAL, std::string("tmjx_lstm_seq_bwd: ") + why);
  const LstmBwd P{a->dh, a->ldd, a->Wh, a->ldw, a->gates, a->c, a->ldo, a->c0, a->ld0, a->reset, a->ldr, a->dgates, a->dh0, a->dc0, a->T, a->rows};
  hipStream_t s = (hipStream_t)stream;
  switch (a->H) {
    case 32: return launch_bwd<32>(P, s);
    case 64: return launch_bwd<64>(P, s);
    case 128: return launch_bwd<128>(P, s);
    default: return launch_bwd<256>(P, s);
  }
}
}
