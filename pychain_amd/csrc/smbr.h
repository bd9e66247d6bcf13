// smbr.h - launch interface of lattice-free sMBR (smbr.hip; include/pychain_hip.h: pychain_hip_smbr_*): the frame
// accuracies of a reference under the denominator's occupancies, and the accuracy-weighted recursions whose products are the
// gradient of the expected accuracy.  Beside the pdf-level form the same by class (§3.27: phone-level accuracy, one silence class).
#ifndef PYCHAIN_HIP_SMBR_H_
#define PYCHAIN_HIP_SMBR_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pychain_hip {

constexpr size_t kSmbrLdsBudget = 160 * 1024;       // the LDS of one CU

// the denominator graph in the reference layout (one graph for every sequence), and its arcs ordered by pdf
struct SmbrGraph {
  const int32_t *ft, *fi; const float* fp;          // arcs {src, dst, pdf} in runs by source, [H][2] run bounds, probabilities
  const int32_t *bt, *bi; const float* bp;          // the same arcs in runs by destination
  const float *leaky, *init, *fin;                  // [H]
  const int32_t *parc, *pidx;                       // [K] ids into ft / fp, stable by pdf; [D + 1] run bounds
  int H, K;
};

struct SmbrAccArgs {
  const float* gamma;        // [B,T,D] the denominator's occupancies, fp32
  const int64_t* lengths;
  const int32_t* pdfs;       // [B,T,Kt]: < 0 padding, >= D counted
  const float* probs;        // [B,T,Kt]
  float* frame_acc;          // [B,T] out: e(b,t) of the live frames
  double* acc_per_seq;       // [B] out
  int32_t* bad_count;        // [2], zeroed on the stream before the launch; [1] += live entries with pdf >= D
  int B, T, D, Kt;
};

struct SmbrArgs {
  SmbrGraph g;
  const void* x; int x_half;             // [B,T,D] raw: kXF32 / kXBf16 / kXF16 (device_utils.h)
  const int64_t* lengths;
  const int32_t* pdfs; const float* probs;
  const float* frame_acc;                // [B,T] from the accuracy pass
  float coef, grad_scale; const float* grad_scale_dev;
  void* grad;                            // [B,T,D] out, x's type
  double* acc_per_seq;                   // [B]: NaN for a sequence that went bad
  float* closing;                        // [B] out
  int32_t* bad_count;                    // [2]: [0] += the sequences that went bad
  float *al, *ab, *be, *bb;              // workspace: [B][T+1][H] alpha', alpha-bar', beta', beta-bar', normalised per frame
  float *tot_a, *tot_b;                  // workspace: [B][T+1] the frame totals divided out - DIAGNOSTIC ONLY: written, read by no kernel
  int32_t* seq_bad;                      // workspace: [2][B], zeroed on the stream before the launches: what the recursions found;
                                         // the verdict claimed (smbr.hip: smbr_condemn)
  int B, T, D, Kt;
};

// Accuracy by CLASS: A(t,n) = Acls(t, cls[n]), Acls(t,c) = the sum of the frame's q_k whose class is c - the
// class of entry k is cls[id_k], or id_k itself where the targets name classes.  A row of x A is then dense.  The class kernels
// take this beside the pdf-level argument structs, which keep their layout.
struct SmbrClasses {
  const int32_t* cls;        // [D] pdf -> class, every value in [0, C) (NOT checked: device memory)
  int C;
  int targets_are_classes;   // the ids of the targets are classes: >= C counted, instead of pdfs: >= D counted
  double* frame_e;           // workspace of the accuracy pass: [B,T] e(b,t) in fp64, live frames only
};

size_t smbr_recursion_lds(int H, int D);            // bytes of LDS the recursion workgroup needs
size_t smbr_grad_lds(int H, int D);
size_t smbr_recursion_lds(int H, int D, int C);     // ... the class form: one table [C] more
size_t smbr_grad_lds(int H, int D, int C);
size_t smbr_lds_bytes(int H, int D, int C);         // the larger of the two, static LDS included; C = 0: the pdf-level form
hipError_t launch_smbr_frame_acc(const SmbrAccArgs& a, hipStream_t st);
hipError_t launch_smbr_frame_acc(const SmbrAccArgs& a, const SmbrClasses& c, hipStream_t st);   // the dense pass, then the per-sequence sums
hipError_t launch_smbr(const SmbrArgs& a, const SmbrClasses& c, hipStream_t st);     // the recursion launch, then the gradient launch; c.cls null: the pdf-level kernels

// The general kernels (smbr_general.hip): any H, D, C.  What the LDS kernels keep in LDS beside the state vectors
// - the frame's row x, its companion x A, the class table; the two D-rows of the gradient - lies in scratch rows of the workspace,
// one set per workgroup, behind the trajectories.
struct SmbrGeneral {
  float* rec;                // [2 B][rec_stride]: x [2][D], x A [2][D], Acls [C] of a recursion workgroup
  float* grad;               // [grad_wgs][grad_stride]: x q0 [D], x (q1 + a q0) [D], Acls [C] of a gradient workgroup
  size_t rec_stride, grad_stride;       // floats, multiples of 64
  int grad_wgs;              // workgroups of the gradient launch, persistent over the (sequence, frame-block) items
  int state_lds;             // 1: the state vectors double-buffered in LDS ("rows"); 0: read back from the trajectories ("global")
};
constexpr int kSmbrGradMaxWgs = 512;                // two gradient workgroups a CU: bounds the scratch
size_t smbr_general_lds(int H);                     // bytes of LDS of the rows form, static LDS included
size_t smbr_general_rec_stride(int D, int C);       // floats
size_t smbr_general_grad_stride(int D, int C);
int smbr_general_grad_wgs(int B, int T);
// the recursion launch, then the gradient launch; c.cls null: the pdf-level form
hipError_t launch_smbr_general(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st);

}  // namespace pychain_hip
#endif
