// Instantiations of the fused conv-stack kernel for one backbone kind (split per kind so the
// translation units compile in parallel).  See conv_stack.hip.h.
#include "conv_stack.hip.h"
namespace wekws {
template int launch_conv_stack_kind<KIND_MDTC>(const Route&, int, const StackParams&, const CallArgs&, hipStream_t);
}  // namespace wekws
