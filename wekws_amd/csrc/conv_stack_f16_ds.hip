// Instantiations of the split-precision (3 x fp16 MFMA) conv-stack kernel for one backbone kind.
// See conv_stack_f16.hip.h.
#include "conv_stack_f16.hip.h"
namespace wekws {
template int launch_conv_stack_f16_kind<KIND_DS>(const Route&, int, const StackParams&, const CallArgs&, hipStream_t);
}  // namespace wekws
