// The forms of the attention kernels, listed ONCE for attention.hip, attention_bf16.hip and attention_dh.hip.
//
// A form is the kernel's text (attention_body.h, attention_bf16_body.h, attention_dh_body.h) compiled under a set of flags; each flag
// adds trailing parameters, always in the order  lens | key_seg, query_mask | key_bias | pick, want:
//   PM_ATTN_LENS  lens (device int32 [B]): the key count is per IMAGE -- lens[b], read once per workgroup and clamped to [1, Nkv];
//                 Nkv stays the launch-wide upper bound and Nkv_pad the layout, so image b computes what it computes alone with
//                 Nkv = lens[b]
//   PM_ATTN_SEG   key_seg (device uint8 [B, Nkv]: segment 0..31 of a key, 255 = padding), query_mask (device uint32 [B, Nq]: bit s =
//                 the query attends to segment s): the key SET is per QUERY -- key k takes part in query q's softmax iff
//                 key_seg[b,k] < 32 and bit key_seg[b,k] of query_mask[b,q] is set; a query with no allowed key gets a finite row
//                 
//   PM_ATTN_BIAS  key_bias (device f32 [B, Nkv]), beside PM_ATTN_SEG: log(weight) of a key in the kernel's score unit -- octaves when
//                 EXP2, nats otherwise --, added to an allowed key's score BEFORE the maximum is taken; -inf = the key is padding
//                 
//   PM_ATTN_PICK  pick (device uint8 [B]: the kind of every image), want, beside PM_ATTN_LENS or PM_ATTN_SEG: a workgroup whose image
//                 has pick[b] != want returns at once and leaves the image's output rows as they are, every other one runs its
//                 twin's text; one launch per kind fills one output buffer
// A compile-time variant by TEXT, not by a template parameter or an inlined body function: the plain form is then the kernel the
// library had before the others existed, token for token -- same symbol, same instruction stream, same registers (a shared
// __device__ body, even force-inlined, was measured to move the schedule of every instantiation).
//
// Included plainly (common.h does) this file gives the list: PM_ATTN_FORMS(X) calls X(form, suffix, trailing arguments...) per form,
// the arguments read from a PmAttnArgs named `a`.  A .hip file that defines
//   PM_ATTN_BODY           its body header, as an #include operand
//   PM_ATTN_NAME(suffix)   its kernel of that suffix
//   PM_ATTN_INSTANTIATE    "include the body once per form, here"
// and includes this file again gets its seven kernels, and launches them through a switch over PmAttnForm built from the same list.
#ifndef PM_ATTENTION_FORMS_H
#define PM_ATTENTION_FORMS_H

#define PM_ATTN_ARGS_SEG a.key_seg, a.query_mask
#define PM_ATTN_ARGS_PICK a.pick, a.want
// the forms whose key set is per image ...
#define PM_ATTN_FORMS_IMAGE(X)                    \
    X(PLAIN, _)                                   \
    X(LENS, _lens_, a.lens)                       \
    X(LENS_PICK, _lens_pick_, a.lens, PM_ATTN_ARGS_PICK)
// ... and per query
#define PM_ATTN_FORMS_QUERY(X)                                                     \
    X(SEG, _seg_, PM_ATTN_ARGS_SEG)                                                \
    X(SEG_PICK, _seg_pick_, PM_ATTN_ARGS_SEG, PM_ATTN_ARGS_PICK)                   \
    X(SEG_BIAS, _seg_bias_, PM_ATTN_ARGS_SEG, a.key_bias)                          \
    X(SEG_BIAS_PICK, _seg_bias_pick_, PM_ATTN_ARGS_SEG, a.key_bias, PM_ATTN_ARGS_PICK)
#define PM_ATTN_FORMS(X) PM_ATTN_FORMS_IMAGE(X) PM_ATTN_FORMS_QUERY(X)

#define PM_ATTN_FORM_ENUM(form, ...) PM_FORM_##form,
enum PmAttnForm { PM_ATTN_FORMS(PM_ATTN_FORM_ENUM) };
#undef PM_ATTN_FORM_ENUM

#endif  // PM_ATTENTION_FORMS_H

#ifdef PM_ATTN_INSTANTIATE
#undef PM_ATTN_INSTANTIATE

#define PM_ATTN_KERNEL PM_ATTN_NAME(_)
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL

#define PM_ATTN_KERNEL PM_ATTN_NAME(_lens_)
#define PM_ATTN_LENS 1
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS

#define PM_ATTN_KERNEL PM_ATTN_NAME(_seg_)
#define PM_ATTN_SEG 1
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL
#undef PM_ATTN_SEG

#define PM_ATTN_KERNEL PM_ATTN_NAME(_lens_pick_)
#define PM_ATTN_LENS 1
#define PM_ATTN_PICK 1
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL
#undef PM_ATTN_LENS
#undef PM_ATTN_PICK

#define PM_ATTN_KERNEL PM_ATTN_NAME(_seg_pick_)
#define PM_ATTN_SEG 1
#define PM_ATTN_PICK 1
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL
#undef PM_ATTN_SEG
#undef PM_ATTN_PICK

#define PM_ATTN_KERNEL PM_ATTN_NAME(_seg_bias_)
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS

#define PM_ATTN_KERNEL PM_ATTN_NAME(_seg_bias_pick_)
#define PM_ATTN_SEG 1
#define PM_ATTN_BIAS 1
#define PM_ATTN_PICK 1
#include PM_ATTN_BODY
#undef PM_ATTN_KERNEL
#undef PM_ATTN_SEG
#undef PM_ATTN_BIAS
#undef PM_ATTN_PICK

#endif  // PM_ATTN_INSTANTIATE
