// CommandKFinger.h — `fpmash kfinger`: the CFL k-finger lines of sequence records (lyn2vec
// `--type basic --type_factorization CFL`, fingerprint_utils.py:95-110, 443-476), written as the
// text `sketch -fp` reads, or with -S sketched straight into the .msh that text would give.
#pragma once

#include "Command.h"

namespace fpmhost {

class CommandKFinger : public Command {
public:
    CommandKFinger();
    int run() const override;
};

}  // namespace fpmhost
