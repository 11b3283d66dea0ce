// Return codes of the C ABI (host only: common.h and the host-only conv_plan.h both need them).
#pragma once
#define TG_OK 0
#define TG_ERR_ARG (-1)
#define TG_ERR_SHAPE (-2)
#define TG_ERR_ALIGN (-3)
#define TG_ERR_HIP (-100)
